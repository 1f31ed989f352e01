// layout_dump_main.cpp -- stand-alone host program: digests of everything sf_build_layout / sf_build_mlp_layout produce, over a
// fixed matrix of shapes.  tests/test_cpu_layout_frozen.py compares its output with tests/golden/layout_digests.txt (recorded by
// scripts/make_layout_golden.py), which freezes every table and descriptor byte of the layout builder.
//   layout_dump                one line per case, then a "summary" line of feature counts
//   layout_dump --tables KEY   one digest per table of the flow case KEY
// Build: g++ -O2 -std=c++17 -I<csrc> layout_dump_main.cpp sf_layout.cpp
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "sf_layout.h"
#include "sf_trainc.h"   // (sf_trc_slots_needed: the part of the header that needs no HIP)

namespace {

struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void bytes(const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  }
  template <class V> void vec(const std::vector<V>& v) {
    const uint64_t n = v.size();
    bytes(&n, sizeof(n));
    if (n) bytes(v.data(), n * sizeof(V));
  }
};

struct Case {
  int kind, D, C, H, T, NB, K, bf16, pm;  // pm: 0 = perms null, 1 = reversed, 2 = shuffled per transform, 3 = NOT a permutation
  std::string key() const {
    char b[96];
    std::snprintf(b, sizeof(b), "%s-D%d-C%d-H%d-T%d-NB%d-K%d-b%d-p%d", kind == SF_MAF ? "maf" : kind == SF_NSF ? "nsf" : "bad", D, C, H,
                  T, NB, K, bf16, pm);
    return b;
  }
};

// every table of a flow layout, by name (the descriptors are "tables" of raw bytes)
template <class F> void each_table(const SfLayout& L, F f) {
  auto raw = [&](const char* n, const void* p, size_t sz) { Fnv h; h.bytes(p, sz); f(n, h.h); };
  auto vec = [&](const char* n, const auto& v) { Fnv h; h.vec(v); f(n, h.h); };
  raw("dev", &L.dev, sizeof(L.dev)); raw("trc", &L.trc, sizeof(L.trc));
  raw("nsc", &L.nsc, sizeof(L.nsc)); raw("nsfS", &L.nsfS, sizeof(L.nsfS));
  vec("src1", L.src1); vec("src2", L.src2); vec("srcT1", L.srcT1); vec("srcT2", L.srcT2); vec("gdst", L.gdst);
  vec("srcB", L.srcB); vec("src16a", L.src16a); vec("src16b", L.src16b); vec("src16B", L.src16B);
  vec("src16c", L.src16c); vec("src16h", L.src16h); vec("srcC1", L.srcC1); vec("srcC2", L.srcC2);
  vec("gdstC", L.gdstC); vec("cst", L.cst);
}

bool build(const Case& c, SfLayout& L) {
  std::memset(&L.dev, 0, sizeof(L.dev)); std::memset(&L.trc, 0, sizeof(L.trc));
  std::memset(&L.nsc, 0, sizeof(L.nsc)); std::memset(&L.nsfS, 0, sizeof(L.nsfS));
  std::vector<float> tm(SF_DMAX + 1), ts(SF_DMAX + 1), xm(513), xs(513);
  for (size_t i = 0; i < tm.size(); ++i) { tm[i] = 0.25f * (float)i - 1.f; ts[i] = 0.5f + 0.125f * (float)i; }
  for (size_t i = 0; i < xm.size(); ++i) { xm[i] = 0.5f * (float)(i % 7) - 1.5f; xs[i] = 0.75f + 0.0625f * (float)(i % 11); }
  std::vector<int32_t> perms((size_t)(c.T > 0 ? c.T : 1) * (c.D > 0 ? c.D : 1));
  uint32_t s = 12345u + (uint32_t)c.D * 977u + (uint32_t)c.T;
  for (int t = 0; t < c.T; ++t) {
    int32_t* p = perms.data() + (size_t)t * c.D;
    for (int j = 0; j < c.D; ++j) p[j] = c.pm == 1 ? c.D - 1 - j : j;
    if (c.pm == 2)
      for (int j = c.D - 1; j > 0; --j) {
        s = s * 1664525u + 1013904223u;
        std::swap(p[j], p[(s >> 8) % (uint32_t)(j + 1)]);
      }
    if (c.pm == 3 && t == c.T - 1) p[c.D - 1] = p[0];
  }
  sf_flow_desc d;
  std::memset(&d, 0, sizeof(d));
  d.kind = c.kind; d.D = c.D; d.C = c.C; d.H = c.H; d.T = c.T; d.K = c.K; d.NB = c.NB;
  d.scale_fn = 0; d.hidden_bf16 = c.bf16;
  d.tail_bound = 3.f; d.min_bin_width = d.min_bin_height = d.min_derivative = 1e-3f; d.maf_eps = d.lu_eps = 1e-3f;
  d.theta_mean = tm.data(); d.theta_std = ts.data(); d.x_mean = xm.data(); d.x_std = xs.data();
  d.perms = c.pm ? perms.data() : nullptr;
  d.ar_slope = 1e-3f;
  return sf_build_layout(d, L);
}

// gsrcC / gzeroC (the gather's tables) against gdstC: every parameter with a position appears exactly once in the position table,
// at its position; every parameter without one exactly once in the zero list.  (Not digested: the golden file predates them.)
bool gather_tables_consistent(const SfLayout& L) {
  if (L.gsrcC.size() != (size_t)L.n_gradC * 2 || L.gdstC.size() != (size_t)L.n_params) return false;
  std::vector<int> in_src((size_t)L.n_params, 0), in_zero((size_t)L.n_params, 0);
  for (size_t k = 0; k < L.gsrcC.size(); ++k) {
    const int32_t i = L.gsrcC[k];
    if (i < 0) continue;
    if (i >= L.n_params || L.gdstC[(size_t)i] != (int32_t)(k / 2)) return false;
    ++in_src[(size_t)i];
  }
  for (int32_t i : L.gzeroC) {
    if (i < 0 || i >= L.n_params) return false;
    ++in_zero[(size_t)i];
  }
  for (size_t i = 0; i < (size_t)L.n_params; ++i)
    if (in_src[i] != (L.gdstC[i] >= 0 ? 1 : 0) || in_zero[i] != (L.gdstC[i] >= 0 ? 0 : 1)) return false;
  return true;
}

std::vector<Case> flow_cases() {
  std::vector<Case> v;
  const int Ds[] = {1, 2, 3, 4, 5, 6, 8, 9, 16}, Cs[] = {1, 8, 10, 30, 41}, Hs[] = {1, 17, 50, 64, 69, 80, 128};
  const int Ts[] = {1, 3}, NBs[] = {1, 2, 4}, Ks[] = {2, 8, 11, 16};
  // the full grid thinned by a stride coprime to every axis: each axis value still meets every other one
  int i = 0;
  for (int D : Ds) for (int C : Cs) for (int H : Hs) for (int T : Ts) for (int NB : NBs) {
    if (i++ % 11 == 0) v.push_back({SF_MAF, D, C, H, T, NB, 0, 0, (i / 11) % 3});
    if (T == 3 && NB == 2 && i % 8 == 0) v.push_back({SF_MAF, D, C, H, T, NB, 0, 1, (i / 8) % 3});
  }
  i = 0;
  for (int D : Ds) for (int C : Cs) for (int H : Hs) for (int T : Ts) for (int NB : NBs) for (int K : Ks) {
    if (i++ % 53 == 0) v.push_back({SF_NSF, D, C, H, T, NB, K, 0, 0});
    if (T == 3 && NB == 2 && i % 29 == 0) v.push_back({SF_NSF, D, C, H, T, NB, K, 1, 0});
  }
  // hand-picked: the shapes the kernels are instantiated for, and what the thinned grid may miss
  for (int D = 3; D <= 5; ++D)
    for (int NB = 1; NB <= 2; ++NB)
      for (int H : {16, 24, 32, 40, 48, 50, 64})
        for (int T : {1, 5}) v.push_back({SF_MAF, D, 10, H, T, NB, 0, 0, T == 5 ? 2 : 0});
  for (int H : {16, 32, 48, 64}) v.push_back({SF_MAF, 4, 8, H, 3, 2, 0, 0, 1});    // cooperative MAF: NT = 1 .. 4 (H = 48: three full groups)
  for (int C : {1, 8, 14, 15, 30}) v.push_back({SF_MAF, 8, C, 64, 2, 2, 0, 0, 2});  // ... NI = 1 / 2; D = 8, H = 64: span placement
  for (int D : {6, 7, 8}) for (int H : {50, 60, 64}) v.push_back({SF_MAF, D, 10, H, 3, 2, 0, 0, 2});
  for (int K : {2, 8, 9, 10, 11})                                                   // cooperative NSF: OTQ 6 / 8, NT 1 .. 5, NI 1 .. 3
    for (int H : {16, 50, 64, 69, 80})
      for (int C : {1, 8, 9, 24, 25, 40}) v.push_back({SF_NSF, 2 + (H + C) % 7, C, H, 1 + (K & 1) * 2, 2, K, 0, 0});
  for (int H : {32, 50, 69, 96, 128}) for (int NB : {1, 2, 4}) v.push_back({SF_NSF, 1, 10, H, 2, NB, 10, 0, 0});  // NSF, D = 1
  for (int H : {50, 64, 69, 128}) for (int NB : {1, 2}) v.push_back({SF_NSF, 5, 30, H, 5, NB, 10, H != 69, 0});   // bf16 NSF / sampler image
  v.push_back({SF_MAF, 8, 41, 128, 3, 4, 0, 1, 0});   // hidden_bf16 over the LDS budget
  v.push_back({SF_NSF, 8, 41, 128, 3, 4, 8, 1, 0});
  // invalid descs: the error strings are frozen too
  v.push_back({SF_MAF, 5, 10, 50, 3, 2, 0, 0, 3});    // perms is not a permutation
  v.push_back({SF_MAF, 2, 10, 50, 1, 2, 0, 0, 3});
  v.push_back({SF_NSF, 5, 10, 50, 3, 2, 1, 0, 0});
  v.push_back({SF_NSF, 5, 10, 50, 3, 2, 17, 0, 0});
  v.push_back({7, 5, 10, 50, 3, 2, 8, 0, 0});
  for (int D : {0, 17}) v.push_back({SF_MAF, D, 10, 50, 3, 2, 0, 0, 0});
  for (int C : {0, 513}) v.push_back({SF_MAF, 5, C, 50, 3, 2, 0, 0, 0});
  for (int H : {0, 129}) v.push_back({SF_NSF, 5, 10, H, 3, 2, 8, 0, 0});
  for (int T : {0, 65}) v.push_back({SF_MAF, 5, 10, 50, T, 2, 0, 0, 0});
  for (int NB : {0, 5}) v.push_back({SF_NSF, 5, 10, 50, 3, NB, 8, 0, 0});
  return v;
}

void mlp_cases() {
  const int shapes[][5] = {{1, 1}, {1, 32}, {1, 33}, {1, 128}, {2, 33, 128}, {2, 1, 32}, {3, 128, 33, 1}, {3, 32, 32, 33},
                           {4, 32, 33, 128, 1}, {4, 128, 128, 128, 128}, {4, 1, 1, 1, 1}, {2, 129, 1}, {2, 32, 0}};
  std::vector<float> xm(512), xs(512);
  for (size_t i = 0; i < xm.size(); ++i) { xm[i] = 0.125f * (float)(i % 13); xs[i] = 1.f + 0.25f * (float)(i % 5); }
  for (int n_in : {1, 41, 512, 0, 513})
    for (const auto& sh : shapes)
      for (int norm = 0; norm < 2; ++norm) {
        if (n_in != 41 && (norm || sh[0] != 1 || sh[1] != 32)) continue;   // (other input widths: one layer, for the n_in checks)
        const int act = (sh[0] + norm) % 3;   // (the activation only lands in the descriptor)
        sf_mlp_desc d;
        std::memset(&d, 0, sizeof(d));
        d.n_in = n_in; d.n_layers = sh[0]; d.act = act;
        for (int l = 0; l < sh[0]; ++l) d.widths[l] = sh[1 + l];
        d.x_mean = norm ? xm.data() : nullptr; d.x_std = norm ? xs.data() : nullptr;
        SfMlpLayout L;
        std::memset(&L.dev, 0, sizeof(L.dev));
        const bool ok = sf_build_mlp_layout(d, L);
        Fnv h;
        h.bytes(&L.dev, sizeof(L.dev));
        h.vec(L.src1); h.vec(L.src2); h.vec(L.srcT1); h.vec(L.srcT2); h.vec(L.gdst); h.vec(L.cst);
        std::printf("mlp-in%d-L%d-w%d.%d.%d.%d-a%d-n%d %s %" PRId64 " %" PRId64 " %" PRId64 " %016" PRIx64 "\n", n_in, sh[0], d.widths[0],
                    d.widths[1], d.widths[2], d.widths[3], act, norm, ok ? "ok" : ("\"" + L.error + "\"").c_str(), L.n_params,
                    L.n_packed, L.n_packedT, h.h);
      }
  for (int extra = 0; extra < 2; ++extra) {   // n_layers / activation out of range
    sf_mlp_desc d;
    std::memset(&d, 0, sizeof(d));
    d.n_in = 4; d.n_layers = extra ? 5 : 1; d.act = extra ? 0 : 3; d.widths[0] = 8;
    SfMlpLayout L;
    const bool ok = sf_build_mlp_layout(d, L);
    std::printf("mlp-bad%d %s\n", extra, ok ? "ok" : ("\"" + L.error + "\"").c_str());
  }
}

}  // namespace

int main(int argc, char** argv) {
  const std::vector<Case> cases = flow_cases();
  if (argc == 3 && std::string(argv[1]) == "--tables") {
    for (const Case& c : cases)
      if (c.key() == argv[2]) {
        SfLayout L;
        const bool ok = build(c, L);
        std::printf("%s %s\n", argv[2], ok ? "ok" : L.error.c_str());
        each_table(L, [](const char* n, uint64_t h) { std::printf("  %-7s %016" PRIx64 "\n", n, h); });
        return 0;
      }
    std::fprintf(stderr, "no such case: %s\n", argv[2]);
    return 2;
  }
  std::map<std::string, int> seen;
  std::vector<std::pair<std::string, int>> feat;   // summary counts, in a fixed order
  auto count = [&](const char* name, bool on) {
    for (auto& f : feat)
      if (f.first == name) { f.second += on ? 1 : 0; return; }
    feat.emplace_back(name, on ? 1 : 0);
  };
  for (const Case& c : cases) {
    if (seen[c.key()]++) continue;   // (a hand-picked shape that the grid holds already)
    SfLayout L;
    const bool ok = build(c, L);
    // one 64-bit digest over everything, and one hex digit per table (in the order of --tables): the digest is the check, the
    // digits tell which table moved
    Fnv all;
    std::string sig;
    each_table(L, [&](const char*, uint64_t h) { all.bytes(&h, sizeof(h)); sig += "0123456789abcdef"[h >> 60]; });
    std::printf("%s %s %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %016" PRIx64 " %s\n",
                c.key().c_str(), ok ? "ok" : ("\"" + L.error + "\"").c_str(), L.n_params, L.n_packed, L.n_packedT, L.n_packedB,
                L.n_packed16, L.n_packed16B, L.n_imgC, L.n_gradC, all.h, sig.c_str());
    if (ok && (L.trc.ok || L.nsc.ok) && !gather_tables_consistent(L)) {
      std::fprintf(stderr, "%s: gsrcC / gzeroC do not match gdstC\n", c.key().c_str());
      return 1;
    }
    const SfDev& v = L.dev;
    const bool maf = ok && c.kind == SF_MAF, nsf = ok && c.kind == SF_NSF;
    bool straddle = false;
    for (int g = 0; g < SF_DMAX; ++g) straddle = straddle || v.g_lo[g] != v.g_tile[g];
    count("maf32_aligned", maf && c.D >= 2 && !straddle);
    count("maf32_contig", maf && straddle);
    count("m16_whole", maf && v.m16_ok && !v.m16_span);
    count("m16_k3", maf && v.m16_ok && v.m16_k3 > 0);
    count("m16_span", maf && v.m16_ok && v.m16_span);
    for (int D = 3; D <= 5; ++D)
      count(("compact_d" + std::to_string(D)).c_str(), maf && c.D == D && !L.src16c.empty() && !L.src16h.empty());
    for (int n = 1; n <= 4; ++n) count(("trc_nt" + std::to_string(n)).c_str(), maf && L.trc.ok && L.trc.NT == n);
    for (int n = 1; n <= 2; ++n) count(("trc_ni" + std::to_string(n)).c_str(), maf && L.trc.ok && L.trc.NI == n);
    count("trc_span_slots6", maf && L.trc.ok && v.m16_span && sf_trc_slots_needed(L.trc) > 5);
    count("nsc_otq6", nsf && L.nsc.ok && L.nsc.OTQ == 6);
    count("nsc_otq8", nsf && L.nsc.ok && L.nsc.OTQ == 8);
    count("nsc_nt5", nsf && L.nsc.ok && L.nsc.NT == 5);
    for (int n = 1; n <= 3; ++n) count(("nsc_ni" + std::to_string(n)).c_str(), nsf && L.nsc.ok && L.nsc.NI == n);
    count("nsfS_parts1", nsf && L.nsfS.ok && L.nsfS.n_parts == 1);
    count("nsfS_parts2", nsf && L.nsfS.ok && L.nsfS.n_parts == 2);
    count("nsfS_off", nsf && !L.nsfS.ok);
    count("dev_parts0", ok && v.n_parts == 0);
    count("bf16_accepted", ok && c.bf16);
    count("bf16_rejected", !ok && c.bf16 && L.error.compare(0, 11, "hidden_bf16") == 0);
    count("t1", ok && c.T == 1);
    count("t_multi", ok && c.T >= 2);
    count("nb1", ok && c.NB == 1);
    count("nb4", ok && c.NB == 4);
    count("nsf_d1", nsf && c.D == 1);
    count("perms_null", maf && c.pm == 0);
    count("bad_perms", !ok && c.pm == 3);
    count("bad_k", !ok && c.kind == SF_NSF && L.error.compare(0, 2, "K ") == 0);
  }
  mlp_cases();
  std::printf("summary cases=%zu", seen.size());
  for (const auto& f : feat) std::printf(" %s=%d", f.first.c_str(), f.second);
  std::printf("\n");
  return 0;
}
