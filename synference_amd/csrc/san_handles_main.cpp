// san_handles_main.cpp -- stand-alone check of who owns the handles' device memory (make san-handles), for the AddressSanitizer +
// UBSan build of the library.  This program DEFINES the HIP entry points the library imports (symbols of the executable come
// first): allocations are malloc-backed and tracked, copies and memsets are real (so ASan checks their bounds), launches do
// nothing.  Every handle kind is driven through its lazily-building entry points; then, for every step and every k, the k-th
// acquisition (hipMalloc, hipHostMalloc, hipEventCreate) inside that step is made to fail: the step must return SF_ERR_HIP, an
// immediate retry SF_OK, and after destroy nothing may be live.  (sf_flow_train_epoch goes on without its two optional buffers: it
// must return SF_OK even then.)  Needs no GPU; never run on one.
//   san_handles_host            the whole check
//   san_handles_host success    the success paths only; with SF_FAKE_HIP_LOG=<file>: one "function bytes" line per runtime call
//                               (frees of one destroy sorted, frees of null left out; a launch carries its kernel's mangled name)
//                               -- equal logs = equal call sequences
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "synference_hip.h"

// ---- the fake runtime ---------------------------------------------------------------------------
static std::map<void*, size_t> g_dev, g_pin;
static std::set<void*> g_ev;
static std::map<std::string, long> g_hits;
static long g_acq = 0, g_fail_at = 0;   // acquisitions since the last arm(); the g_fail_at-th fails (0: none)
static int failures = 0;
static FILE* g_log = nullptr;
static bool g_in_destroy = false;
static std::vector<std::string> g_destroy_frees;

static void hit(const char* fn, size_t bytes = 0, bool is_free = false, const char* detail = "") {
  ++g_hits[fn];
  if (!g_log) return;
  const std::string line = std::string(fn) + detail + " " + std::to_string(bytes) + "\n";
  if (is_free && g_in_destroy) g_destroy_frees.push_back(line);
  else std::fputs(line.c_str(), g_log);
}
static bool acquire() { return ++g_acq != g_fail_at; }
static hipError_t release(std::map<void*, size_t>& live, void* p, const char* fn) {
  if (!p) { ++g_hits[fn]; return hipSuccess; }
  auto it = live.find(p);
  if (it == live.end()) { std::printf("FAILED: %s of a pointer that is not live\n", fn); std::abort(); }
  hit(fn, it->second, true);
  live.erase(it);
  std::free(p);
  return hipSuccess;
}
static dim3 g_grid, g_block;
static size_t g_shmem;
static hipStream_t g_stream;

extern "C" {
hipError_t hipMalloc(void** p, size_t n) {
  hit("hipMalloc", n);
  if (!acquire()) { *p = nullptr; return hipErrorOutOfMemory; }
  *p = n ? std::malloc(n) : nullptr;
  if (*p) g_dev[*p] = n;
  return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) {
  hit("hipHostMalloc", n);
  if (!acquire()) { *p = nullptr; return hipErrorOutOfMemory; }
  *p = std::malloc(n);
  g_pin[*p] = n;
  return hipSuccess;
}
hipError_t hipFree(void* p) { return release(g_dev, p, "hipFree"); }
hipError_t hipHostFree(void* p) { return release(g_pin, p, "hipHostFree"); }
hipError_t hipEventCreate(hipEvent_t* e) {
  hit("hipEventCreate");
  if (!acquire()) { *e = nullptr; return hipErrorOutOfMemory; }
  *e = (hipEvent_t)std::malloc(1);
  g_ev.insert(*e);
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t e) {
  if (!g_ev.erase(e)) { std::printf("FAILED: hipEventDestroy of an event that is not live\n"); std::abort(); }
  hit("hipEventDestroy", 0, true);
  std::free(e);
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { hit("hipEventRecord"); return g_ev.count(e) ? hipSuccess : hipErrorInvalidHandle; }
hipError_t hipEventSynchronize(hipEvent_t e) { hit("hipEventSynchronize"); return g_ev.count(e) ? hipSuccess : hipErrorInvalidHandle; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
  hit("hipEventElapsedTime");
  *ms = 0.f;
  return g_ev.count(a) && g_ev.count(b) ? hipSuccess : hipErrorInvalidHandle;
}
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { hit("hipMemcpy", n); if (n) std::memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) { hit("hipMemcpyAsync", n); if (n) std::memmove(d, s, n); return hipSuccess; }
hipError_t hipMemset(void* d, int v, size_t n) { hit("hipMemset", n); if (n) std::memset(d, v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) { hit("hipMemsetAsync", n); if (n) std::memset(d, v, n); return hipSuccess; }
hipError_t hipGetDeviceCount(int* n) { hit("hipGetDeviceCount"); *n = 1; return hipSuccess; }
hipError_t hipGetDevice(int* d) { hit("hipGetDevice"); *d = 0; return hipSuccess; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t* p, int) {   // (the header maps the name to the versioned symbol the library imports)
  hit("hipGetDeviceProperties");
  std::memset(p, 0, sizeof *p);
  p->multiProcessorCount = 256;
  return hipSuccess;
}
const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory (injected)" : "fake runtime error"; }
hipError_t hipGetLastError(void) { ++g_hits["hipGetLastError"]; return hipSuccess; }
hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int v) { hit("hipFuncSetAttribute", (size_t)v); return hipSuccess; }
hipError_t hipOccupancyMaxActiveBlocksPerMultiprocessor(int* n, const void*, int, size_t) { hit("hipOccupancyMaxActiveBlocksPerMultiprocessor"); *n = 1; return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { hit("hipStreamSynchronize"); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { hit("hipStreamCreateWithFlags"); *s = nullptr; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t) { hit("hipStreamDestroy"); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { hit("hipStreamWaitEvent"); return hipSuccess; }
// host stub -> mangled kernel name.  (Function-local: the library's module constructors register their kernels before this
// program's own globals are constructed.)
static std::map<const void*, std::string>& kernel_names() { static auto* m = new std::map<const void*, std::string>(); return *m; }
hipError_t hipLaunchKernel(const void* fn, dim3 g, dim3 b, void**, size_t sh, hipStream_t) {
  hit("hipLaunchKernel", (size_t)g.x * g.y * g.z * b.x * b.y * b.z + sh, false, (" " + kernel_names()[fn]).c_str());   // (threads + dynamic LDS: the launch shape)
  return hipSuccess;
}
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t sh, hipStream_t st) { g_grid = g; g_block = b; g_shmem = sh; g_stream = st; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* g, dim3* b, size_t* sh, hipStream_t* st) { *g = g_grid; *b = g_block; *sh = g_shmem; *st = g_stream; return hipSuccess; }
void** __hipRegisterFatBinary(const void*) { static void* h[1]; return h; }
void __hipRegisterFunction(void**, const void* stub, char*, const char* name, unsigned, void*, void*, void*, void*, int*) { kernel_names()[stub] = name; }
void __hipUnregisterFatBinary(void**) {}
}  // extern "C"

// ---- the checks ---------------------------------------------------------------------------------
#define EXPECT(cond, what)                                                                                       \
  do {                                                                                                           \
    if (!(cond)) { std::printf("FAILED %s:%d: %s: %s [%s]\n", __FILE__, __LINE__, (what).c_str(), #cond, sf_last_error()); ++failures; } \
  } while (0)

static std::vector<float> g_flat(1 << 20, 0.01f), g_theta(256 * 16, 0.1f), g_x(256 * 32, 0.2f), g_out(40 * 2000 * 16), g_grad(1 << 20),
    g_loss(256), g_dctx(256 * 32), g_lo(16, -3.f), g_hi(16, 3.f);
static std::vector<float> g_m(1 << 20), g_v(1 << 20);
static std::vector<int64_t> g_rows(256);
static std::vector<int32_t> g_drawn(64);
static const std::vector<uint32_t> g_slots = {0, 3, 4, 9, 14};   // (of the 3 x 5 output slots, sorted)

struct Scenario {
  std::string name;
  std::function<void*()> create;
  std::function<void(void*)> destroy;
  struct Step { std::string first; std::function<int(void*)> second; int rc_on_failure = SF_ERR_HIP; };
  std::vector<Step> steps;
};

static void destroy_checked(const Scenario& sc, void* h, const std::string& what) {
  g_in_destroy = true;
  sc.destroy(h);
  g_in_destroy = false;
  std::sort(g_destroy_frees.begin(), g_destroy_frees.end());
  for (auto& l : g_destroy_frees) std::fputs(l.c_str(), g_log);
  g_destroy_frees.clear();
  EXPECT(g_dev.empty() && g_pin.empty() && g_ev.empty(), what + ": live after destroy: " + std::to_string(g_dev.size()) + " device, " +
                                                             std::to_string(g_pin.size()) + " pinned, " + std::to_string(g_ev.size()) + " events");
  for (auto& kv : g_dev) std::free(kv.first);
  for (auto& kv : g_pin) std::free(kv.first);
  for (void* e : g_ev) std::free(e);
  g_dev.clear(); g_pin.clear(); g_ev.clear();
}
static void arm(long k) { g_acq = 0; g_fail_at = k; }

// success run: acquisitions per step
static std::vector<long> run_success(const Scenario& sc) {
  std::vector<long> acq;
  if (g_log) std::fprintf(g_log, "## %s\n", sc.name.c_str());
  void* h = sc.create();
  for (auto& st : sc.steps) {
    if (g_log) std::fprintf(g_log, "# %s\n", st.first.c_str());
    arm(0);
    EXPECT(st.second(h) == SF_OK, sc.name + " / " + st.first);
    acq.push_back(g_acq);
  }
  if (g_log) std::fprintf(g_log, "# destroy\n");
  destroy_checked(sc, h, sc.name + " (no failure)");
  return acq;
}
static long run_injected(const Scenario& sc, const std::vector<long>& acq) {
  long cases = 0;
  for (size_t s = 0; s < sc.steps.size(); ++s)
    for (long k = 1; k <= acq[s]; ++k, ++cases) {
      const std::string what = sc.name + " / " + sc.steps[s].first + " / acquisition " + std::to_string(k) + " of " + std::to_string(acq[s]);
      void* h = sc.create();
      for (size_t i = 0; i < s; ++i) EXPECT(sc.steps[i].second(h) == SF_OK, what + ": earlier step " + sc.steps[i].first);
      arm(k);
      EXPECT(sc.steps[s].second(h) == sc.steps[s].rc_on_failure, what + ": the step with the failure");
      if (sc.steps[s].rc_on_failure == SF_ERR_HIP) {   // the message names the runtime function and carries the runtime's error string
        const char* m = sf_last_error();                // (sf_opt_create reports its allocations and memsets under its own name)
        EXPECT((std::strstr(m, "hipMalloc") || std::strstr(m, "hipHostMalloc") || std::strstr(m, "hipEventCreate") || std::strstr(m, "sf_opt_create")) &&
                   std::strstr(m, "out of memory (injected)"), what + ": error message");
      }
      arm(0);
      for (size_t i = s; i < sc.steps.size(); ++i) EXPECT(sc.steps[i].second(h) == SF_OK, what + ": retry / later step " + sc.steps[i].first);
      destroy_checked(sc, h, what);
    }
  return cases;
}

static Scenario flow_scenario(const std::string& name, int kind, int D, int C, int NB, bool profiling = true) {
  Scenario sc;
  sc.name = name;
  sc.create = [=]() -> void* {
    static const std::vector<float> zero(512, 0.f), one(512, 1.f);
    sf_flow_desc d;
    std::memset(&d, 0, sizeof d);
    d.kind = kind; d.D = D; d.C = C; d.H = 50; d.T = 5; d.K = 8; d.NB = NB;
    d.tail_bound = kind == SF_NSF_AR || kind == SF_MAF_AR ? 5.f : 3.f;
    d.min_bin_width = d.min_bin_height = d.min_derivative = d.maf_eps = d.lu_eps = d.ar_slope = 1e-3f;
    d.theta_mean = zero.data(); d.theta_std = one.data(); d.x_mean = zero.data(); d.x_std = one.data();
    sf_flow* f = nullptr;
    if (sf_flow_create(&d, &f) != SF_OK || !f) { std::printf("FAILED: sf_flow_create(%s): %s\n", name.c_str(), sf_last_error()); std::exit(1); }
    sf_flow_set_profiling(f, profiling);   // (on: the training events are created too)
    return f;
  };
  sc.destroy = [](void* h) { sf_flow_destroy((sf_flow*)h); };
  const bool plain = kind == SF_MAF || (kind == SF_NSF && D > 1);
  auto F = [](void* h) { return (sf_flow*)h; };
  auto set_params = [=](void* h) { return sf_flow_set_params(F(h), g_flat.data(), sf_flow_num_params(F(h)), 0, nullptr); };
  auto sample = [=](int64_t M, int64_t S, int32_t max_attempts = 0) {
    return [=](void* h) {
      int64_t unfilled = -1;
      return sf_flow_sample(F(h), g_x.data(), M, S, g_lo.data(), g_hi.data(), 7, max_attempts, g_out.data(), g_drawn.data(), &unfilled, nullptr);
    };
  };
  auto loss_grad = [=](int64_t B, bool dctx, bool rows) {
    return [=](void* h) {
      if (plain && (sf_flow_train_path(F(h), B, dctx) == 0) != dctx) {   // (the step must run the path its name says)
        std::printf("FAILED: %s, B = %ld: training path %d\n", name.c_str(), (long)B, sf_flow_train_path(F(h), B, dctx));
        ++failures;
      }
      if (rows) return sf_flow_loss_grad_rows(F(h), g_flat.data(), g_theta.data(), g_x.data(), g_rows.data(), B, 1.f, nullptr, g_loss.data(), nullptr,
                                              g_grad.data(), nullptr, nullptr);
      return sf_flow_loss_grad_weighted(F(h), g_flat.data(), g_theta.data(), g_x.data(), B, 1.f, nullptr, g_loss.data(), g_grad.data(),
                                        dctx ? g_dctx.data() : nullptr, nullptr);
    };
  };
  sc.steps.push_back({"set_params", set_params});
  sc.steps.push_back({"log_prob", [=](void* h) { return sf_flow_log_prob(F(h), g_theta.data(), g_x.data(), 100, g_loss.data(), nullptr); }});
  sc.steps.push_back({"sample 3x5", sample(3, 5)});
  sc.steps.push_back({"sample 40x2000", sample(40, 2000)});   // (more than 2^16 slots: the retry ring grows too)
  if (plain) sc.steps.push_back({"sample 3x5, at most 2048 attempts", sample(3, 5, 2048)});   // (the capped schedule)
  sc.steps.push_back({"sample_slots 5 of 3x5", [=](void* h) {
                        int64_t unfilled = -1;
                        return sf_flow_sample_slots(F(h), g_x.data(), 3, 5, g_slots.data(), (int64_t)g_slots.size(), g_lo.data(), g_hi.data(), 7, 0,
                                                    g_out.data(), &unfilled, nullptr);
                      }});
  sc.steps.push_back({"acceptance 3x100", [=](void* h) {
                        return sf_flow_acceptance(F(h), g_x.data(), 3, 100, g_lo.data(), g_hi.data(), 7, g_drawn.data(), nullptr);
                      }});
  sc.steps.push_back({"inverse_from_noise 100", [=](void* h) {
                        return sf_flow_inverse_from_noise(F(h), g_theta.data(), g_x.data(), 100, g_out.data(), g_loss.data(), nullptr);
                      }});
  sc.steps.push_back({"inverse_from_noise_sampler 100", [=](void* h) {   // (positive: which arithmetic ran, not an error)
                        const int rc = sf_flow_inverse_from_noise_sampler(F(h), g_theta.data(), g_x.data(), 100, g_out.data(), nullptr);
                        return rc > 0 ? (int)SF_OK : rc;
                      }});
  sc.steps.push_back({"get_params", [=](void* h) { return sf_flow_get_params(F(h), g_grad.data(), sf_flow_num_params(F(h)), 0, nullptr); }});
  if (plain) {
    sc.steps.push_back({"prepare_context 3", [=](void* h) { return sf_flow_prepare_context(F(h), g_x.data(), 3, nullptr); }});
    sc.steps.push_back({"prepare_context 200", [=](void* h) { return sf_flow_prepare_context(F(h), g_x.data(), 200, nullptr); }});
    sc.steps.push_back({"log_prob_grad", [=](void* h) {
                          return sf_flow_log_prob_grad(F(h), g_theta.data(), g_x.data(), 1, 64, g_loss.data(), g_grad.data(), nullptr);
                        }});
    sc.steps.push_back({"loss_grad 32 (cooperative)", loss_grad(32, false, false)});
    sc.steps.push_back({"loss_grad 200 (cooperative)", loss_grad(200, false, false)});
    sc.steps.push_back({"loss_grad 32 (generic)", loss_grad(32, true, false)});
    sc.steps.push_back({"loss_grad 200 (generic)", loss_grad(200, true, false)});
  } else {
    sc.steps.push_back({"loss_grad 32", loss_grad(32, false, false)});
    sc.steps.push_back({"loss_grad_rows 200", loss_grad(200, false, true)});
  }
  sc.steps.push_back({"train_epoch 2 x 32", [=](void* h) {   // (the batch size of an earlier step: only the optional buffers are new)
                        const sf_adam_desc ad = {1e-3f, 0.9f, 0.999f, 1e-8f, 0.f, 0};
                        static float scratch[2];
                        static double loss_sum;
                        return sf_flow_train_epoch(F(h), g_flat.data(), g_theta.data(), g_x.data(), g_rows.data(), 2, 32, 1.f, g_m.data(), g_v.data(), &ad,
                                                   0, 1.f, scratch, g_grad.data(), &loss_sum, nullptr);
                      }, SF_OK});
  if (profiling && !(kind == SF_NSF && D == 1))   // (the one-parameter NSF brackets nothing)
    sc.steps.push_back({"train_stats", [=](void* h) { float ms; return sf_flow_train_stats(F(h), &ms); }});
  return sc;
}

int main(int argc, char** argv) {
  const bool success_only = argc > 1 && std::strcmp(argv[1], "success") == 0;
  if (const char* p = std::getenv("SF_FAKE_HIP_LOG")) g_log = std::fopen(p, "w");
  if (!g_log) g_log = std::fopen("/dev/null", "w");
  for (size_t i = 0; i < g_rows.size(); ++i) g_rows[i] = (int64_t)(i % 200);

  std::vector<Scenario> all;
  all.push_back(flow_scenario("maf D=5", SF_MAF, 5, 20, 2));
  all.push_back(flow_scenario("nsf D=4", SF_NSF, 4, 10, 2));
  all.push_back(flow_scenario("nsf D=1", SF_NSF, 1, 10, 2));
  all.push_back(flow_scenario("nsf_ar D=3", SF_NSF_AR, 3, 10, 2));
  all.push_back(flow_scenario("maf_ar D=3", SF_MAF_AR, 3, 10, 2));
  all.push_back(flow_scenario("maf D=5, profiling off", SF_MAF, 5, 20, 2, false));   // (the training launches without their event bracket)
  all.push_back(flow_scenario("nsf D=4, profiling off", SF_NSF, 4, 10, 2, false));
  {
    Scenario sc;
    sc.name = "mlp";
    sc.create = []() -> void* {
      static const std::vector<float> zero(64, 0.f), one(64, 1.f);
      sf_mlp_desc d;
      std::memset(&d, 0, sizeof d);
      d.n_in = 10; d.n_layers = 3; d.widths[0] = 50; d.widths[1] = 50; d.widths[2] = 8; d.act = SF_ACT_RELU;
      d.x_mean = zero.data(); d.x_std = one.data();
      sf_mlp* m = nullptr;
      if (sf_mlp_create(&d, &m) != SF_OK || !m) { std::printf("FAILED: sf_mlp_create: %s\n", sf_last_error()); std::exit(1); }
      return m;
    };
    sc.destroy = [](void* h) { sf_mlp_destroy((sf_mlp*)h); };
    sc.steps.push_back({"forward 100", [](void* h) { return sf_mlp_forward((sf_mlp*)h, g_flat.data(), g_x.data(), 100, g_out.data(), nullptr); }});
    for (int64_t B : {32, 200})
      sc.steps.push_back({"backward " + std::to_string(B), [B](void* h) {
                            return sf_mlp_backward((sf_mlp*)h, g_flat.data(), g_x.data(), g_out.data(), B, g_grad.data(), nullptr);
                          }});
    all.push_back(sc);
  }
  {   // (the optimiser allocates in its create: the "handle" of the scenario is a slot for it)
    Scenario sc;
    sc.name = "opt";
    sc.create = []() -> void* { return new sf_opt*(nullptr); };
    sc.destroy = [](void* h) { sf_opt_destroy(*(sf_opt**)h); delete (sf_opt**)h; };
    sc.steps.push_back({"create", [](void* h) {
                          sf_adam_desc d = {1e-3f, 0.9f, 0.999f, 1e-8f, 0.f, 0};
                          if (*(sf_opt**)h) return (int)SF_OK;
                          return sf_opt_create(1000, &d, (sf_opt**)h);
                        }});
    sc.steps.push_back({"adam_step", [](void* h) { return sf_adam_step(*(sf_opt**)h, g_flat.data(), g_grad.data(), 1.f, nullptr, nullptr); }});
    all.push_back(sc);
  }

  long cases = 0;
  for (auto& sc : all) {
    const std::vector<long> acq = run_success(sc);
    long tot = 0;
    for (long a : acq) tot += a;
    std::printf("%-24s success path: %ld acquisitions over %zu steps\n", sc.name.c_str(), tot, sc.steps.size());
    if (!success_only) cases += run_injected(sc, acq);
  }
  // every fake the script is meant to reach was reached (a fake that is never called checks nothing)
  for (const char* fn : {"hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree", "hipEventCreate", "hipEventDestroy", "hipEventRecord",
                         "hipEventSynchronize", "hipEventElapsedTime", "hipMemcpy", "hipMemcpyAsync", "hipMemset", "hipMemsetAsync",
                         "hipGetDeviceCount", "hipGetDevice", "hipGetDeviceProperties", "hipGetLastError", "hipFuncSetAttribute",
                         "hipOccupancyMaxActiveBlocksPerMultiprocessor", "hipStreamSynchronize", "hipLaunchKernel"})
    EXPECT(g_hits[fn] > 0, std::string("fake never reached: ") + fn);
  std::fclose(g_log);
  if (failures) std::printf("san_handles: %d check(s) failed\n", failures);
  else std::printf("san_handles: all checks passed (%ld injected failures)\n", cases);
  return failures ? 1 : 0;
}
