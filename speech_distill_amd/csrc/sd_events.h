// Timing-disabled hipEvent_t sets leased per call and per device from a small process-wide pool (the only process state of
// the stream-ordering helpers): two concurrent calls -- different host threads, different devices -- never share an event,
// and nothing is created on the steady-state path.  An event may be re-recorded by a later call while a wait enqueued by
// an earlier one is still pending: hipStreamWaitEvent captures the record that was current when it was issued.
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include <vector>
#include "../../include/sd_hip.h"

constexpr int kSdEventsPerSet = 12;
struct SdEventSet {
  hipEvent_t ev[kSdEventsPerSet];
  int device;
};
SdEventSet* sd_lease_events();
void sd_return_events(SdEventSet* s);

// What each event of a set is for, one name per purpose.  sd_qwen3_backward (main = `stream`, side = opts->side_stream):
enum SdBwdEvent {
  // main records when the named buffer is final, side waits before the weight-gradient GEMM that reads it
  kEvGradIn = 0,  // the gradient entering the head (dlogits) or a layer (dx_in): lm_head dW, down-projection dW
  kEvDgu = 1,     // d(gate|up): gate|up dW (separate-GEMM schedule only)
  kEvDxb = 2,     // gradient of the post-attention residual: o-projection dW (separate-GEMM schedule only)
  kEvDqkv = 3,    // d(q|k|v), the last input of a layer's dW: q|k|v dW, or the grouped launch of all four
  // 4, 5: free
  kEvGainPartials = 6,  // main records after the layer's last norm backward; side waits before the batched gain reduce
  kEvSideDrained = 7,   // side records, main waits: all side was given so far (head, separate-GEMM layer, end of call)
  kEvLentNorm = 8,      // lent to sd_rmsnorm_bwd2 / _slabs (post-attention norm): main records there, side waits, reduces
  kEvLentQkNorm = 9,    // lent to sd_qknorm_rope_bwd2: the same for the q / k gain reduces
  kEvLayerDone = 10,    // + the layer's parity (10, 11): side records behind the layer's grouped dW (and batched gain
                        // reduce); main waits in the next layer, before it overwrites their inputs and before the callback
};
// sd_attn_bwd2 / sd_attn_bwd_varlen under attn.bwd_split (a set of their own; the default single launch needs none)
enum SdAttnEvent {
  kEvAttnInputs = 0,  // main records when delta is final; side waits before the dQ kernel
  kEvAttnDq = 1,      // side records behind the dQ kernel; main waits before the entry returns
};

// `to` will run after everything `from` has been given so far (0, or SD_ERR_WORKSPACE when a HIP call fails)
static inline int sd_order_after(hipStream_t from, hipStream_t to, hipEvent_t ev) {
  return hipEventRecord(ev, from) != hipSuccess || hipStreamWaitEvent(to, ev, 0) != hipSuccess ? SD_ERR_WORKSPACE : 0;
}

// The two streams of a call and its leased events.  Without a side stream every operation is a no-op returning 0.
struct SdStreamOrder {
  hipStream_t main = nullptr, side = nullptr;
  SdEventSet* set = nullptr;  // leased by init(), returned when the call ends
  ~SdStreamOrder() { if (set) sd_return_events(set); }
  int init(void* main_stream, void* side_stream) {
    main = (hipStream_t)main_stream, side = (hipStream_t)side_stream;
    return side && !(set = sd_lease_events()) ? SD_ERR_WORKSPACE : 0;
  }
  hipEvent_t event(int e) const { return side ? set->ev[e] : nullptr; }  // also: what is lent to a *_bwd2 entry
  int side_waits_for_main(int e) const { return side ? sd_order_after(main, side, event(e)) : 0; }
  int main_waits_for_side(int e) const { return side ? sd_order_after(side, main, event(e)) : 0; }
  // the two halves of main_waits_for_side, for a wait that is enqueued later than the record
  int record_on_side(int e) const { return side && hipEventRecord(event(e), side) != hipSuccess ? SD_ERR_WORKSPACE : 0; }
  int main_waits_for_record(int e) const {
    return side && hipStreamWaitEvent(main, event(e), 0) != hipSuccess ? SD_ERR_WORKSPACE : 0;
  }
};
