"""sd_sample_step_rows against its yardstick, the existing sd_sample_step run on each row ALONE with that row's own
parameters and its own uniform pair.  Every comparison is torch.equal: the per-row entry runs the same kernels, instantiated
over where the parameters come from.  V = 2056: three 1024-column blocks with a ragged last one, eight score slices."""
import ctypes as C

import pytest
import torch

from gpu_util import dev

pytestmark = pytest.mark.gpu

V, B, CAP = 2056, 6, 64
X, Y = 700, 1900            # two heavy tokens in different 1024-column blocks
SHAPE, ALIGN, WORKSPACE = -1, -2, -5


@pytest.fixture(scope="module")
def ops():
    import speech_distill_amd as sda
    sda.load_lib()
    from speech_distill_amd import ops as o
    return o


def _logits(seed):
    g = torch.Generator().manual_seed(seed)
    lg = 2.0 * torch.randn(B, V, generator=g)
    lg[3, X], lg[3, Y] = 14.0, 13.0     # the RAS row: X is the likely candidate, Y the runner-up of the raw softmax
    lg[0, 77] = 30.0                    # the greedy row's arg-max is its EOS, suppressed by min_new_tokens
    lg[1, 78] = 30.0                    # the top_k = 1 row takes its EOS
    return lg.to(torch.bfloat16)


def _mixed(ops):
    """Six rows: greedy, top_k = 1, top_k = 20 / top_p = 0.8, top_k = 128 with RAS (fallback forced), top_k = 0, finished."""
    P = ops.sample_params
    return [
        P(do_sample=False, temperature=0.9, repetition_penalty=1.5, min_new_tokens=6, eos_token_id=77, pad_token_id=1),
        P(do_sample=True, temperature=0.7, top_k=1, repetition_penalty=1.1, min_new_tokens=2, eos_token_id=78, pad_token_id=2),
        P(do_sample=True, temperature=1.3, top_k=20, top_p=0.8, repetition_penalty=1.25, min_new_tokens=0, eos_token_id=5,
          pad_token_id=3),
        P(do_sample=True, temperature=0.5, top_k=128, top_p=0.95, repetition_penalty=1.0, min_new_tokens=1, eos_token_id=9,
          pad_token_id=4, use_ras=True, win_size=10, tau_r=0.4),
        P(do_sample=True, temperature=0.8, top_k=0, repetition_penalty=1.2, min_new_tokens=3, eos_token_id=11, pad_token_id=5),
        P(do_sample=True, temperature=1.1, top_k=50, top_p=0.9, repetition_penalty=1.3, eos_token_id=12, pad_token_id=6),
    ]


def _state(lg):
    """Histories that touch each row's largest logits (so the penalty moves candidates); row 3 holds X four times in its
    last ten tokens (4 + 1 >= ceil(10 * 0.4)); row 5 is finished."""
    g = torch.Generator().manual_seed(3)
    prompt_len = [3, 5, 2, 4, 6, 3]
    gen_len = [2, 3, 7, 9, 4, 1]
    seq = torch.zeros(B, CAP, dtype=torch.int64)
    for b in range(B):
        n = prompt_len[b] + gen_len[b]
        seq[b, :n] = torch.randint(0, V, (n,), generator=g)
        top = torch.topk(lg[b].float(), 4).indices
        seq[b, prompt_len[b]] = top[1]
        seq[b, n - 1] = top[2]
    seq[3, 5:13:2] = X
    pl = torch.tensor(prompt_len, dtype=torch.int32)
    ln = pl + torch.tensor(gen_len, dtype=torch.int32)
    fin = torch.tensor([0, 0, 0, 0, 0, 1], dtype=torch.uint8)
    return seq, pl, ln, fin


def _uniforms(u_stride, seed=5):
    g = torch.Generator().manual_seed(seed)
    U = torch.rand(B, u_stride, 2, generator=g)
    return U


def _alone(ops, lg, u_pair, seq, pl, ln, fin, sp, b):
    """The yardstick: sd_sample_step on row b alone.  -> (seq row, len, finished, next, pos)."""
    s, l, f = seq[b:b + 1].clone().to(dev()), ln[b:b + 1].clone().to(dev()), fin[b:b + 1].clone().to(dev())
    nxt, pos = ops.sample_step(lg[b:b + 1].contiguous().to(dev()), u_pair.reshape(1, 2).contiguous().to(dev()), s,
                               pl[b:b + 1].clone().to(dev()), l, f, sp)
    return s[0].cpu(), int(l[0]), int(f[0]), int(nxt[0]), int(pos[0])


def _rows(ops, lg, U, seq, pl, ln, fin, params, max_new, env=None):
    s, l, f = seq.clone().to(dev()), ln.clone().to(dev()), fin.clone().to(dev())
    lgd = lg.to(dev())
    keep = lgd.clone()
    nxt, pos = ops.sample_step_rows(lgd, U.to(dev()), s, pl.to(dev()), l, f, ops.sample_params_rows(params, dev()),
                                    torch.tensor(max_new, dtype=torch.int32, device=dev()), env or ops.sample_env(params))
    torch.cuda.synchronize()
    assert torch.equal(lgd, keep)                      # the raw logits survive
    return s.cpu(), l.cpu(), f.cpu(), nxt.cpu(), pos.cpu()


def _same_as_alone(ops, lg, U, seq, pl, ln, fin, params, got):
    s, l, f, nxt, pos = got
    for b in range(B):
        g = int(ln[b] - pl[b])
        ws, wl, wf, wn, wp = _alone(ops, lg, U[b, g], seq, pl, ln, fin, params[b], b)
        assert torch.equal(s[b], ws), b
        assert (int(l[b]), int(f[b]), int(nxt[b]), int(pos[b])) == (wl, wf, wn, wp), b


def test_mixed_rows_equal_each_row_alone(ops):
    lg, params = _logits(1), _mixed(ops)
    seq, pl, ln, fin = _state(lg)
    U = _uniforms(16)
    U[3, int(ln[3] - pl[3])] = torch.tensor([0.3, 0.8])      # candidate X; then X from the processed row, not from the raw
    env = ops.sample_env(params)
    assert (env.max_top_k, env.any_sample, env.any_ras, env.any_full) == (128, 1, 1, 1)
    got = _rows(ops, lg, U, seq, pl, ln, fin, params, [100] * B)
    _same_as_alone(ops, lg, U, seq, pl, ln, fin, params, got)
    s, l, f, nxt, pos = got
    assert int(nxt[0]) != 77 and int(f[0]) == 0               # greedy: EOS suppressed by its own min_new_tokens
    assert int(nxt[1]) == 78 and int(f[1]) == 1               # top_k = 1: its own EOS ends it
    assert int(nxt[5]) == 6 and int(l[5]) == int(ln[5]) and torch.equal(s[5], seq[5])   # finished: its own pad, no change
    # the RAS row really took the fallback: without RAS the same uniforms give X, with it the raw softmax gives another
    no_ras = ops.sample_params(do_sample=True, temperature=0.5, top_k=128, top_p=0.95, min_new_tokens=1, eos_token_id=9,
                               pad_token_id=4)
    assert _alone(ops, lg, U[3, int(ln[3] - pl[3])], seq, pl, ln, fin, no_ras, 3)[3] == X and int(nxt[3]) != X
    # one step serves both full-vocabulary sources: swap rows 3 and 4 and nothing changes but the order
    perm = [0, 1, 2, 4, 3, 5]
    got2 = _rows(ops, lg[perm], U[perm], seq[perm], pl[perm], ln[perm], fin[perm], [params[i] for i in perm], [100] * B)
    assert torch.equal(got2[3], nxt[perm]) and torch.equal(got2[0], s[perm])


def test_identical_rows_equal_one_sample_step(ops):
    lg = _logits(2)
    seq, pl, ln, fin = _state(lg)
    U = _uniforms(12, seed=6)
    for sp in (ops.sample_params(do_sample=True, temperature=0.6, top_k=100, top_p=0.9, repetition_penalty=1.25,
                                 min_new_tokens=8, eos_token_id=7, pad_token_id=1, use_ras=True, win_size=25, tau_r=0.2),
               ops.sample_params(do_sample=True, temperature=0.8, top_k=0, repetition_penalty=1.25, pad_token_id=1),
               ops.sample_params(do_sample=False, repetition_penalty=1.25, pad_token_id=1)):
        u = torch.stack([U[b, int(ln[b] - pl[b])] for b in range(B)])
        s, l, f = seq.clone().to(dev()), ln.clone().to(dev()), fin.clone().to(dev())
        nxt, pos = ops.sample_step(lg.to(dev()), u.to(dev()), s, pl.to(dev()), l, f, sp)
        got = _rows(ops, lg, U, seq, pl, ln, fin, [sp] * B, [100] * B)
        for a, b in zip(got, (s, l, f, nxt, pos)):
            assert torch.equal(a, b.cpu())


def test_budget_ends_a_row_exactly_at_max_new_and_the_uniform_index_follows_the_row(ops):
    """Three steps on the same logits, no EOS anywhere.  Row b has generated gen[b] tokens when the test starts and its
    budget leaves it 1, 2, 3, 50, 2 and 1 more: it finishes exactly there, not before.  Every step's pair is U[b, len -
    prompt_len], which moves with the row: the yardstick is handed exactly that pair."""
    P = ops.sample_params
    lg = _logits(4)
    params = [P(do_sample=True, temperature=1.0, top_k=40, pad_token_id=1), P(do_sample=True, top_k=1, pad_token_id=2),
              P(do_sample=True, temperature=1.3, top_k=20, top_p=0.8, repetition_penalty=1.25, pad_token_id=3),
              P(do_sample=True, temperature=0.5, top_k=128, top_p=0.95, pad_token_id=4, use_ras=True, win_size=10, tau_r=0.4),
              P(do_sample=True, temperature=0.8, top_k=0, repetition_penalty=1.2, pad_token_id=5),
              P(do_sample=False, repetition_penalty=1.3, pad_token_id=6)]
    seq, pl, ln, fin = _state(lg)
    fin[5] = 0
    gen = (ln - pl).tolist()
    left = [1, 2, 3, 50, 2, 1]
    max_new = [g + k for g, k in zip(gen, left)]
    U = _uniforms(16, seed=8)
    dp, dm = ops.sample_params_rows(params, dev()), torch.tensor(max_new, dtype=torch.int32, device=dev())
    s, l, f = seq.clone().to(dev()), ln.clone().to(dev()), fin.clone().to(dev())
    env = ops.sample_env(params)
    for step in range(3):
        s0, l0, f0 = s.cpu(), l.cpu(), f.cpu()
        nxt, pos = ops.sample_step_rows(lg.to(dev()), U.to(dev()), s, pl.to(dev()), l, f, dp, dm, env)
        for b in range(B):
            g = int(l0[b] - pl[b])
            assert g == gen[b] + min(step, left[b])                 # the pair index is the row's own count
            ws, wl, wf, wn, wp = _alone(ops, lg, U[b, g], s0, pl, l0, f0, params[b], b)
            assert torch.equal(s[b].cpu(), ws) and (int(l[b]), int(nxt[b]), int(pos[b])) == (wl, wn, wp), (step, b)
        assert f.cpu().tolist() == [int(step + 1 >= k) for k in left], step
    assert (l.cpu() - pl).tolist() == [g + min(3, k) for g, k in zip(gen, left)]


def _raw_params(ops, **kw):
    from speech_distill_amd._lib import SampleParams
    base = dict(do_sample=1, top_k=20, use_ras=0, win_size=0, ras_min_count=1, min_new_tokens=0, eos_token_id=-1,
                pad_token_id=0, temperature=1.0, top_p=1.0, repetition_penalty=1.0, pad_=0.0)
    base.update(kw)
    return SampleParams(*[base[n] for n, _ in SampleParams._fields_])


def test_out_of_range_device_parameters_are_clamped(ops):
    """Garbage in the device arrays: top_k = 999, a negative win_size, g >= u_stride, pad / eos past V, temperature <= 0
    and NaN, len past cap, a negative budget.  Nothing is written outside seq[b, :cap] (sentinel rows around the buffer and
    every slot but the row's own), every token lies in [0, V), and a clamped row equals the row with the legal value."""
    from speech_distill_amd._lib import SampleEnv
    lg = _logits(7)
    seq, pl, ln, fin = _state(lg)
    fin[5] = 0
    ln[4] = CAP + 50                      # a length past the row: clamped to cap, the row is full
    ln[2] = CAP - 1                       # the last slot
    pl[2] = 0
    seq[2] = torch.randint(0, V, (CAP,), generator=torch.Generator().manual_seed(1))
    nan = float("nan")
    bad = [_raw_params(ops, top_k=999, temperature=0.7),
           _raw_params(ops, top_k=64, use_ras=1, win_size=-5, ras_min_count=2, top_p=0.9),
           _raw_params(ops, top_k=-3, pad_token_id=10 ** 6, eos_token_id=V + 5, temperature=-1.0, top_p=nan),
           _raw_params(ops, top_k=0, temperature=nan, repetition_penalty=-2.0, win_size=2 ** 31 - 1, use_ras=7),
           _raw_params(ops, top_k=5, pad_token_id=-9),
           _raw_params(ops, do_sample=0, top_k=-1, pad_token_id=10 ** 6)]
    env = SampleEnv(20, 1, 1, 0)          # no full-vocabulary launch from the processed row: top_k = 0 cannot ask for one
    U = _uniforms(2, seed=9)              # u_stride = 2 < every row's generated count but one
    max_new = [100, -5, 100, 100, 100, 0]
    guard = torch.full(((B + 2) * CAP,), -7, dtype=torch.int64, device=dev())
    s = guard[CAP:(B + 1) * CAP].view(B, CAP)
    s.copy_(seq)
    l, f = ln.clone().to(dev()), fin.clone().to(dev())
    nxt, pos = ops.sample_step_rows(lg.to(dev()), U.to(dev()), s, pl.to(dev()), l, f, ops.sample_params_rows(bad, dev()),
                                    torch.tensor(max_new, dtype=torch.int32, device=dev()), env)
    torch.cuda.synchronize()
    g = guard.cpu()
    assert bool((g[:CAP] == -7).all()) and bool((g[(B + 1) * CAP:] == -7).all())
    got = g[CAP:(B + 1) * CAP].view(B, CAP)
    assert bool(((nxt >= 0) & (nxt < V)).all()) and bool(((pos >= 0) & (pos < CAP)).all())
    for b in range(B):
        n = min(int(ln[b]), CAP)
        changed = (got[b] != seq[b]).nonzero().flatten().tolist()
        assert changed in ([], [n]) and (n < CAP or not changed), (b, changed)
    assert int(l[4]) == CAP + 50 and int(f[4]) == 1 and int(nxt[4]) == 0    # full row: finished, pad clamped to 0
    assert int(l[2]) == CAP and int(pos[2]) == CAP - 1                       # the last slot was taken
    assert int(f[1]) == 1 and int(f[5]) == 1                                 # budgets of -5 and 0: spent after one commit
    # clamped = legal: top_k 999 -> the launch's 20 (pair 1, g clamped to u_stride - 1)
    legal = ops.sample_params(do_sample=True, temperature=0.7, top_k=20, pad_token_id=0)
    assert int(nxt[0]) == _alone(ops, lg, U[0, 1], seq, pl, ln, fin, legal, 0)[3]
    # a negative win_size is an empty window: the RAS row draws from its processed candidates (top_k 64 -> 20)
    legal = ops.sample_params(do_sample=True, top_k=20, top_p=0.9, pad_token_id=0)
    assert int(nxt[1]) == _alone(ops, lg, U[1, 1], seq, pl, ln, fin, legal, 1)[3]


def test_host_argument_errors_return_the_codes_before_any_launch(ops):
    import speech_distill_amd as sda
    from speech_distill_amd._lib import SampleEnv
    lib = sda.load_lib()
    nb = lib.sd_sample_workspace_bytes(B, V)
    ws = torch.zeros(nb, dtype=torch.uint8, device=dev())
    lg = _logits(1).to(dev())
    seq, pl, ln, fin = (t.to(dev()) for t in _state(_logits(1)))
    U = _uniforms(4).to(dev())
    params = ops.sample_params_rows(_mixed(ops), dev())
    mn = torch.full((B,), 10, dtype=torch.int32, device=dev())
    nxt, pos = torch.zeros(B, dtype=torch.int64, device=dev()), torch.zeros(B, dtype=torch.int32, device=dev())
    before = (seq.clone(), ln.clone(), fin.clone())

    def call(env=SampleEnv(128, 1, 1, 1), **kw):
        a = dict(logits=lg.data_ptr(), stride=V, u=U.data_ptr(), us=4, seq=seq.data_ptr(), pl=pl.data_ptr(),
                 ln=ln.data_ptr(), fin=fin.data_ptr(), nxt=nxt.data_ptr(), pos=pos.data_ptr(), ws=ws.data_ptr(), nb=nb,
                 params=params.data_ptr(), mn=mn.data_ptr(), B=B, V=V, cap=CAP)
        a.update(kw)
        return lib.sd_sample_step_rows(a["logits"], a["stride"], a["u"], a["us"], a["seq"], a["pl"], a["ln"], a["fin"],
                                       a["nxt"], a["pos"], a["ws"], a["nb"], a["params"], a["mn"],
                                       None if env is None else C.byref(env), a["B"], a["V"], a["cap"], None)

    for name in ("logits", "u", "seq", "pl", "ln", "fin", "nxt", "pos", "params", "mn"):
        assert call(**{name: None}) == SHAPE, name
    assert call(env=None) == SHAPE
    for kw in (dict(B=0), dict(B=65536), dict(V=0), dict(cap=0), dict(us=0), dict(stride=V - 8)):
        assert call(**kw) == SHAPE, kw
    for env in (SampleEnv(129, 1, 0, 0), SampleEnv(-1, 1, 0, 0)):
        assert call(env=env) == SHAPE
    assert call(V=8, stride=8, env=SampleEnv(9, 1, 0, 0)) == SHAPE            # max_top_k > V
    assert call(V=V - 4) == ALIGN and call(stride=V + 4) == ALIGN
    assert call(logits=lg.data_ptr() + 2) == ALIGN and call(ws=ws.data_ptr() + 8) == ALIGN
    assert call(params=params.data_ptr() + 2) == ALIGN
    assert call(nb=nb - 1) == WORKSPACE and call(ws=None) == WORKSPACE
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (seq, ln, fin)))   # nothing ran
    with pytest.raises(ValueError):
        ops.sample_step_rows(lg, U[:, :, :1].contiguous(), seq, pl, ln, fin, params, mn, SampleEnv(128, 1, 1, 1))
    with pytest.raises(ValueError):
        ops.sample_step_rows(lg, U, seq, pl, ln, fin, params[:-1].contiguous(), mn, SampleEnv(128, 1, 1, 1))
