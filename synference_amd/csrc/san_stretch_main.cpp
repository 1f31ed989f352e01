// san_stretch_main.cpp -- stand-alone host check of the ensemble sampler's step (sf_stretch_step) for the AddressSanitizer +
// UBSan build of the library (make san-stretch): every argument check, all of which sit ahead of the launch.  Needs no GPU
// and launches nothing (N = 0 is the one accepted call).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "synference_hip.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::printf("FAILED %s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, sf_last_error()); \
      ++failures;                                                             \
    }                                                                         \
  } while (0)

struct Call {
  int64_t N = 8, D = 5, W = 16, max_fixed = 2;
  float *walkers, *lp, *lo, *hi, *lp_prop, *prop, *out, *out_lp;
  int32_t *fixed, *accepted, *tp = nullptr, *ta = nullptr;
  int64_t S = 100, collect = -1, row_offset = 0, half_step = 3;
  int resolve = 1, propose = 1;
  int run() const {
    return sf_stretch_step(N, D, W, max_fixed, walkers, lp, fixed, lo, hi, lp_prop, prop, accepted, out, out_lp, S, collect, 7u,
                           row_offset, half_step, resolve, propose, tp, ta, nullptr);
  }
};

int main() {
  std::vector<float> f(64 * 64 * 16, 0.f);
  std::vector<int32_t> n(64 * 32, 0);
  Call ok;
  ok.walkers = ok.lp = ok.lo = ok.hi = ok.lp_prop = ok.prop = ok.out = ok.out_lp = f.data();
  ok.fixed = ok.accepted = n.data();

  { Call c = ok; c.N = 0; EXPECT(c.run() == SF_OK); }                      // nothing to do: no launch
  { Call c = ok; c.N = 0; c.walkers = nullptr; EXPECT(c.run() == SF_OK); }
  { Call c = ok; c.N = -1; EXPECT(c.run() == SF_ERR_INVALID); }
  { Call c = ok; c.S = -1; EXPECT(c.run() == SF_ERR_INVALID); }
  { Call c = ok; c.row_offset = -1; EXPECT(c.run() == SF_ERR_INVALID); }
  { Call c = ok; c.half_step = -1; EXPECT(c.run() == SF_ERR_INVALID); }
  { Call c = ok; c.half_step = (int64_t)1 << 32; EXPECT(c.run() == SF_ERR_INVALID); }
  for (int64_t D : {(int64_t)0, (int64_t)-3, (int64_t)17}) {
    Call c = ok; c.D = D; c.max_fixed = 0;
    EXPECT(c.run() == SF_ERR_INVALID && std::strstr(sf_last_error(), "D outside") != nullptr);
  }
  for (int64_t W : {(int64_t)0, (int64_t)2, (int64_t)3, (int64_t)15, (int64_t)63, (int64_t)66, (int64_t)128, (int64_t)-4}) {
    Call c = ok; c.W = W;
    EXPECT(c.run() == SF_ERR_INVALID && std::strstr(sf_last_error(), "walkers") != nullptr);
  }
  // an empty free set, and a bound that is none
  { Call c = ok; c.max_fixed = c.D; EXPECT(c.run() == SF_ERR_INVALID && std::strstr(sf_last_error(), "free set") != nullptr); }
  { Call c = ok; c.D = 1; c.max_fixed = 1; EXPECT(c.run() == SF_ERR_INVALID && std::strstr(sf_last_error(), "free set") != nullptr); }
  { Call c = ok; c.max_fixed = -1; EXPECT(c.run() == SF_ERR_INVALID); }
  { Call c = ok; c.half_step = 0; EXPECT(c.run() == SF_ERR_INVALID && std::strstr(sf_last_error(), "predecessor") != nullptr); }
  // null pointers
  { Call c = ok; c.walkers = nullptr; EXPECT(c.run() == SF_ERR_INVALID); }
  { Call c = ok; c.lp = nullptr; EXPECT(c.run() == SF_ERR_INVALID); }
  { Call c = ok; c.fixed = nullptr; EXPECT(c.run() == SF_ERR_INVALID); }
  { Call c = ok; c.lo = nullptr; EXPECT(c.run() == SF_ERR_INVALID && std::strstr(sf_last_error(), "together") != nullptr); }
  { Call c = ok; c.hi = nullptr; EXPECT(c.run() == SF_ERR_INVALID && std::strstr(sf_last_error(), "together") != nullptr); }
  { Call c = ok; c.lp_prop = nullptr; EXPECT(c.run() == SF_ERR_INVALID); }
  { Call c = ok; c.accepted = nullptr; EXPECT(c.run() == SF_ERR_INVALID); }
  { Call c = ok; c.prop = nullptr; EXPECT(c.run() == SF_ERR_INVALID); }
  { Call c = ok; c.prop = nullptr; c.resolve = 0; EXPECT(c.run() == SF_ERR_INVALID && std::strstr(sf_last_error(), "proposing") != nullptr); }
  { Call c = ok; c.prop = nullptr; c.propose = 0; EXPECT(c.run() == SF_ERR_INVALID && std::strstr(sf_last_error(), "resolving") != nullptr); }
  // collecting
  { Call c = ok; c.collect = 0; c.out = nullptr; EXPECT(c.run() == SF_ERR_INVALID && std::strstr(sf_last_error(), "needs out") != nullptr); }
  { Call c = ok; c.collect = 7; EXPECT(c.run() == SF_ERR_INVALID && std::strstr(sf_last_error(), "beyond") != nullptr); }   // 7 * 16 >= 100
  { Call c = ok; c.collect = 0; c.S = 0; EXPECT(c.run() == SF_ERR_INVALID); }

  std::printf(failures ? "san_stretch: %d check(s) failed\n" : "san_stretch: all checks passed\n", failures);
  return failures ? 1 : 0;
}
