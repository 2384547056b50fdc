// smr_stage.hpp -- host only: the stage clock of a call that reports HIP-event times of its stages (smr_rows_times and its kin).
// StageClock<N_EV, N_MS> owns N_EV events (made at the first begin, destroyed with the clock; not copyable) and the N_MS times of the last
// call.  A call begins the clock where its times start to be its own, marks events on its stream between the stages, and once the stream is
// synchronised turns pairs of events into times.
#pragma once
#include <hip/hip_runtime.h>

struct smr_ctx;
int dev_fail(smr_ctx* c, const char* call, hipError_t e);      // (smr_engine.hip)

template <int N_EV, int N_MS> class StageClock {
  hipEvent_t ev_[N_EV] = {};
  double ms_[N_MS ? N_MS : 1] = {};

 public:
  StageClock() = default;
  StageClock(const StageClock&) = delete;
  StageClock& operator=(const StageClock&) = delete;
  ~StageClock() { for (auto e : ev_) if (e) (void)hipEventDestroy(e); }

  // the events that are not there yet; every time := 0
  int begin(smr_ctx* c) {
    for (auto& e : ev_) if (!e) { const hipError_t r = hipEventCreate(&e); if (r != hipSuccess) { e = nullptr; return dev_fail(c, "hipEventCreate", r); } }
    for (int k = 0; k < N_MS; k++) ms_[k] = 0.0;
    return 0;
  }
  int mark(smr_ctx* c, int i, hipStream_t st) {
    const hipError_t r = hipEventRecord(ev_[i], st);
    return r == hipSuccess ? 0 : dev_fail(c, "hipEventRecord", r);
  }
  // milliseconds from event a to event b (both reached); false, and `ms` as it was, when HIP cannot say
  bool elapsed(int a, int b, double& ms) const {
    float f = 0;
    if (hipEventElapsedTime(&f, ev_[a], ev_[b]) != hipSuccess) return false;
    ms = f;
    return true;
  }
  // time k := / += the milliseconds from event a to event b; as it was when HIP cannot say
  void set(int k, int a, int b) { (void)elapsed(a, b, ms_[k]); }
  void add(int k, int a, int b) { double d; if (elapsed(a, b, d)) ms_[k] += d; }
  void acc(int k, double ms) { ms_[k] += ms; }         // (a time that another clock measured)
  void copy_to(double* out) const { for (int k = 0; k < N_MS; k++) out[k] = ms_[k]; }
};
