// Process-wide runtime bits of the library that are not the executor: the last error of the calling thread (tr_set_error / tr_last_error),
// the launch profiler behind tr_profile_begin / tr_profile_end (tr_prof_note / tr_prof_mark / tr_prof_restart, see tr_common.h) and
// tr_version.
#include <stdarg.h>
#include <string.h>
#include <vector>
#include "tr_common.h"
#include <mutex>

static thread_local char g_err[512] = "";

void tr_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* tr_last_error(void) { return g_err; }

// ---- launch profiler (see tr_common.h) ---------------------------------------------------------------------------------
namespace {
struct ProfRec { char label[48]; double flops, bytes; };
struct Prof {
  std::atomic<bool> on{false};
  hipStream_t st = nullptr;
  std::vector<hipEvent_t> ev;       // ev[0] = begin, ev[i+1] = after mark i
  std::vector<ProfRec> recs;
  size_t used = 0;
};
// ONE recording per process, whatever thread launches: a training step's forward runs on the caller's thread, its backward on the
// autograd engine's device thread, and a recording started by the caller must see both (round 3: per-thread state recorded a third of
// the step).  The launches of a recording are sequential on one stream; the mutex only keeps the vectors consistent.
Prof g_prof;
std::mutex g_prof_mu;
thread_local ProfRec t_note;        // the pending note -> mark pair of this thread's current launch
thread_local bool t_noted = false;
}  // namespace

void tr_prof_note(const char* label, double flops, double bytes) {
  if (!g_prof.on.load(std::memory_order_relaxed)) return;
  snprintf(t_note.label, sizeof(t_note.label), "%s", label);
  t_note.flops = flops;
  t_note.bytes = bytes;
  t_noted = true;
}

void tr_prof_mark(const char* label) {
  Prof& p = g_prof;
  if (!p.on.load(std::memory_order_relaxed)) return;
  ProfRec r;
  if (t_noted) r = t_note;
  else { snprintf(r.label, sizeof(r.label), "%s", label); r.flops = 0; r.bytes = 0; }
  t_noted = false;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (!p.on.load(std::memory_order_relaxed)) return;
  if (p.used + 1 >= p.ev.size()) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    p.ev.push_back(e);
  }
  (void)hipEventRecord(p.ev[p.used + 1], p.st);
  ++p.used;
  p.recs.push_back(r);
}

// Called at the top of the executors: when a recording is active and nothing has been marked yet, the opening event is taken again
// HERE, so the first mark does not include the host time between tr_profile_begin and the executor's first launch.
void tr_prof_restart() {
  Prof& p = g_prof;
  if (!p.on.load(std::memory_order_relaxed)) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (p.on.load(std::memory_order_relaxed) && p.used == 0) (void)hipEventRecord(p.ev[0], p.st);
}

// Start recording the launches the process enqueues on stream s through this library (must not be capturing).
extern "C" int tr_profile_begin(tr_stream_t s) {
  Prof& p = g_prof;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (p.ev.empty()) {
    hipEvent_t e;
    TR_REQUIRE(hipEventCreate(&e) == hipSuccess, TR_ERR_LAUNCH, "tr_profile_begin: cannot create an event");
    p.ev.push_back(e);
  }
  p.st = static_cast<hipStream_t>(s);
  p.recs.clear();
  p.used = 0;
  t_noted = false;
  TR_REQUIRE(hipEventRecord(p.ev[0], p.st) == hipSuccess, TR_ERR_LAUNCH, "tr_profile_begin: event record failed");
  p.on.store(true);
  return TR_OK;
}

// Stop, wait for the stream, and return up to `max` marks: label (48 chars each), ms since the previous mark, FLOPs, bytes.
// Returns the number of marks recorded (may exceed max; only max are written), or < 0 on error.
extern "C" int tr_profile_end(int max, char* labels, float* ms, double* flops, double* bytes) {
  Prof& p = g_prof;
  TR_REQUIRE(p.on.load(), TR_ERR_CONFIG, "tr_profile_end: no recording is active");
  p.on.store(false);
  std::lock_guard<std::mutex> lk(g_prof_mu);
  TR_REQUIRE(hipStreamSynchronize(p.st) == hipSuccess, TR_ERR_LAUNCH, "tr_profile_end: stream synchronize failed");
  const int n = (int)p.recs.size();
  for (int i = 0; i < n && i < max; ++i) {
    float t = 0.f;
    (void)hipEventElapsedTime(&t, p.ev[i], p.ev[i + 1]);
    if (labels) memcpy(labels + (size_t)i * 48, p.recs[i].label, 48);
    if (ms) ms[i] = t;
    if (flops) flops[i] = p.recs[i].flops;
    if (bytes) bytes[i] = p.recs[i].bytes;
  }
  return n;
}
extern "C" int tr_version(void) { return 100; }
