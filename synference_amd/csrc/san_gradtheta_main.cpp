// san_gradtheta_main.cpp -- stand-alone host check of the posterior-mode entry points (sf_flow_log_prob_grad, sf_map_step)
// for the AddressSanitizer + UBSan build of the library (make san-gradtheta): every argument check and state check that is
// reachable without a device, for every flow kind.  Needs no GPU and launches nothing.
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

static sf_flow* make(int kind, int D) {
  static const std::vector<float> zero(512, 0.f), one(512, 1.f);
  sf_flow_desc d;
  std::memset(&d, 0, sizeof d);
  d.kind = kind; d.D = D; d.C = 10; d.H = 50; d.T = 5; d.K = 8; d.NB = 2;
  d.tail_bound = kind == SF_NSF_AR || kind == SF_MAF_AR ? 5.f : 3.f;
  d.min_bin_width = d.min_bin_height = d.min_derivative = d.maf_eps = d.lu_eps = d.ar_slope = 1e-3f;
  d.theta_mean = zero.data(); d.theta_std = one.data(); d.x_mean = zero.data(); d.x_std = one.data();
  sf_flow* f = nullptr;
  EXPECT(sf_flow_create(&d, &f) == SF_OK && f != nullptr);
  return f;
}

int main() {
  std::vector<float> theta(64 * 16, 0.1f), x(64 * 10, 0.2f), lp(64), g(64 * 16);
  EXPECT(sf_flow_log_prob_grad(nullptr, theta.data(), x.data(), 1, 8, lp.data(), g.data(), nullptr) == SF_ERR_INVALID);

  // kinds without the kernel: refused by name before anything else is looked at
  struct { int kind, D; const char* word; } none[] = {{SF_NSF, 1, "one-parameter NSF"}, {SF_NSF_AR, 3, "nsf_ar"}, {SF_MAF_AR, 3, "maf_ar"}};
  for (auto& k : none) {
    sf_flow* f = make(k.kind, k.D);
    if (!f) continue;
    EXPECT(sf_flow_log_prob_grad(f, theta.data(), x.data(), 1, 8, lp.data(), g.data(), nullptr) == SF_ERR_INVALID);
    EXPECT(std::strstr(sf_last_error(), k.word) != nullptr);
    sf_flow_destroy(f);
  }

  // kinds with the kernel: argument and state checks (no parameters are ever set here: there is no device)
  struct { int kind, D; } built[] = {{SF_MAF, 5}, {SF_MAF, 1}, {SF_MAF, 16}, {SF_NSF, 2}, {SF_NSF, 8}};
  for (auto& k : built) {
    sf_flow* f = make(k.kind, k.D);
    if (!f) continue;
    EXPECT(sf_flow_log_prob_grad(f, theta.data(), x.data(), 1, 0, lp.data(), g.data(), nullptr) == SF_OK);
    EXPECT(sf_flow_log_prob_grad(f, theta.data(), x.data(), 1, 8, nullptr, nullptr, nullptr) == SF_OK);
    EXPECT(sf_flow_log_prob_grad(f, theta.data(), x.data(), 1, -1, lp.data(), g.data(), nullptr) == SF_ERR_INVALID);
    EXPECT(sf_flow_log_prob_grad(f, theta.data(), x.data(), 0, 8, lp.data(), g.data(), nullptr) == SF_ERR_INVALID);
    EXPECT(sf_flow_log_prob_grad(f, nullptr, x.data(), 1, 8, lp.data(), g.data(), nullptr) == SF_ERR_INVALID);
    EXPECT(sf_flow_log_prob_grad(f, theta.data(), nullptr, 1, 8, lp.data(), g.data(), nullptr) == SF_ERR_INVALID);
    EXPECT(sf_flow_log_prob_grad(f, theta.data(), x.data(), 7, 8, lp.data(), g.data(), nullptr) == SF_ERR_STATE);
    EXPECT(sf_flow_log_prob_grad(f, theta.data(), x.data(), 1, 8, lp.data(), nullptr, nullptr) == SF_ERR_STATE);
    EXPECT(std::strstr(sf_last_error(), "sf_flow_set_params") != nullptr);
    sf_flow_destroy(f);
  }

  // sf_map_step
  float* t = theta.data();
  EXPECT(sf_map_step(0, 5, t, t, t, t, t, t, t, t, t, t, 0.01f, 1, 1, nullptr) == SF_OK);
  EXPECT(sf_map_step(-1, 5, t, t, t, t, t, t, t, t, t, t, 0.01f, 1, 1, nullptr) == SF_ERR_INVALID);
  EXPECT(sf_map_step(8, 0, t, t, t, t, t, t, t, t, t, t, 0.01f, 1, 1, nullptr) == SF_ERR_INVALID);
  EXPECT(sf_map_step(8, 17, t, t, t, t, t, t, t, t, t, t, 0.01f, 1, 1, nullptr) == SF_ERR_INVALID);
  EXPECT(sf_map_step(8, 5, t, t, t, nullptr, t, t, t, t, t, t, 0.01f, 1, 1, nullptr) == SF_ERR_INVALID);
  EXPECT(sf_map_step(8, 5, t, t, t, t, nullptr, t, t, t, t, t, 0.01f, 1, 1, nullptr) == SF_ERR_INVALID);
  EXPECT(sf_map_step(8, 5, t, t, t, t, t, t, t, t, nullptr, t, 0.01f, 1, 1, nullptr) == SF_ERR_INVALID);
  EXPECT(sf_map_step(8, 5, t, t, t, t, t, t, t, t, t, nullptr, 0.01f, 1, 1, nullptr) == SF_ERR_INVALID);
  EXPECT(sf_map_step(8, 5, nullptr, t, t, t, t, t, t, t, t, t, 0.01f, 1, 1, nullptr) == SF_ERR_INVALID);
  EXPECT(sf_map_step(8, 5, t, nullptr, t, t, t, t, t, t, t, t, 0.01f, 1, 1, nullptr) == SF_ERR_INVALID);
  EXPECT(sf_map_step(8, 5, t, t, nullptr, t, t, t, t, t, t, t, 0.01f, 1, 1, nullptr) == SF_ERR_INVALID);
  EXPECT(sf_map_step(8, 5, t, t, t, t, t, t, t, t, t, t, 0.01f, 0, 1, nullptr) == SF_ERR_INVALID);
  EXPECT(sf_map_step(8, 5, t, t, t, t, t, t, nullptr, t, t, t, 0.01f, 1, 1, nullptr) == SF_ERR_INVALID);
  EXPECT(sf_map_step(8, 5, t, t, t, t, t, t, t, nullptr, t, t, 0.01f, 1, 1, nullptr) == SF_ERR_INVALID);

  std::printf(failures ? "san_gradtheta: %d check(s) failed\n" : "san_gradtheta: all checks passed\n", failures);
  return failures ? 1 : 0;
}
