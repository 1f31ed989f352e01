// sf_layout.cpp -- host-side construction of the MFMA operand image tables.
// Pure host code (no HIP calls): exercised by the CPU test-suite through sf_flow_pack_table(), and frozen table by table
// by tests/test_cpu_layout_frozen.py (layout_dump_main.cpp against tests/golden/layout_digests.txt).
// Logical layout: include/synference_hip.h.  sf_build_layout is LayoutBuilder::run(): one named step per image.
#include "sf_layout.h"

#include <cmath>
#include <cstring>
#include <functional>

namespace {

using Mask = std::function<bool(int, int)>;              // (output row, input row) of a weight block -> connected
using WFn = std::function<int64_t(int, int, int, int)>;  // (ot, ro, it, ri) of a 16-row block -> logical index or -1
using BFn = std::function<int64_t(int, int)>;            // (ot, ro) of a 16-row bias block -> logical index or -1
using Groups = std::vector<std::vector<int>>;            // hidden units of each MADE degree, lowest degree first

struct Emitter {
  std::vector<int32_t>& s1;
  std::vector<int32_t>& s2;
  std::vector<int32_t>* gidx = nullptr;  // gradient-image index of each packed float
  int64_t cur = 0;  // write cursor (floats)

  int64_t pad_to(int64_t align) {
    while (cur % align) push(-1, -1);
    return cur;
  }
  void push(int32_t a, int32_t b, int64_t g = -1) {
    s1.push_back(a);
    s2.push_back(b);
    if (gidx) gidx->push_back((int32_t)(g >= 0 ? g : cur));
    ++cur;
  }
  // Weight block: OT output tiles x nG input groups x 64 lanes x 4.
  // logical index of element (o,i) = base + o*so + i*si ; mask(o,i) false -> structural zero.
  int64_t linear(int OT, int nG, const std::vector<int>& orow, const std::vector<int>& irow,
                 int64_t base, int64_t so, int64_t si, const Mask& mask) {
    int64_t start = cur;
    for (int mt = 0; mt < OT; ++mt)
      for (int kg = 0; kg < nG; ++kg)
        for (int l = 0; l < 64; ++l)
          for (int j = 0; j < 4; ++j) {
            int o = orow[mt * 32 + (l & 31)];
            int i = irow[kg * 8 + 4 * (l >> 5) + j];
            const int64_t g = start + (((int64_t)mt * nG + kg) * 4 + j) * 64 + l;
            if (o >= 0 && i >= 0 && (!mask || mask(o, i)))
              push((int32_t)(base + o * so + i * si), -1, g);
            else
              push(-1, -1, g);
          }
    return start;
  }
  // Bias block [OT][2][16]; up to two logical sources summed (b0 + bc).
  int64_t bias(int OT, const std::vector<int>& orow, int64_t base1, int64_t base2) {
    int64_t start = cur;
    for (int mt = 0; mt < OT; ++mt)
      for (int h = 0; h < 2; ++h)
        for (int r = 0; r < 16; ++r) {
          int o = orow[mt * 32 + sf_tile_row(r, h)];
          const int64_t g = start + mt * 32 + sf_tile_row(r, h);
          if (o >= 0)
            push((int32_t)(base1 + o), base2 >= 0 ? (int32_t)(base2 + o) : -1, g);
          else
            push(-1, -1, g);
        }
    return start;
  }
};

std::vector<int> iota_rows(int n_valid, int n_total) {
  std::vector<int> v(n_total, -1);
  for (int i = 0; i < n_valid && i < n_total; ++i) v[i] = i;
  return v;
}

int ceil_div(int a, int b) { return (a + b - 1) / b; }

// ---- MADE masks: hidden unit j has degree j % max(1, D - 1) + min(1, D - 1); dimension i has degree i + 1 -------------
struct Made {
  int mx, mn;
  explicit Made(int D) : mx(std::max(1, D - 1)), mn(std::min(1, D - 1)) {}
  int deg(int unit) const { return unit % mx + mn; }
  bool in(int unit, int dim) const { return deg(unit) >= dim + 1; }           // first layer: unit <- theta dimension
  bool hid(int out, int in_) const { return deg(out) >= deg(in_); }           // hidden layer: unit <- unit
  bool head(int row, int unit) const { return (row / 2 + 1) > deg(unit); }    // final layer: (a | m) row of a dimension <- unit
  using Fn = bool (Made::*)(int, int) const;
  Mask mask(Fn f) const { const Made m = *this; return [m, f](int o, int i) { return (m.*f)(o, i); }; }
  // the transposed image walks a block with the forward INPUT as its row: same predicate, arguments swapped
  Mask maskT(Fn f) const { const Made m = *this; return [m, f](int i, int o) { return (m.*f)(o, i); }; }
};

// ---- placements of degree groups into tiles of R rows (R = 32: log_prob / training, R = 16: the incremental sampler) --
// whole groups, one after the other, a group never split: fails when a group exceeds a tile or more than 4 tiles are needed
// (what was placed up to there stays)
struct Packed {
  bool ok;
  int last_tile = 0;
  std::vector<int> rows, tile_of, end_of;   // row -> unit; per group: its tile, exclusive end row of the degrees <= its own
};
Packed pack_whole_groups(const Groups& grp, int R, bool enabled) {
  const int G = (int)grp.size();
  Packed p{enabled, 0, std::vector<int>(4 * R, -1), std::vector<int>(G, 0), std::vector<int>(G, 0)};
  int used = 0;
  for (int g = 0; g < G && p.ok; ++g) {
    const int n = (int)grp[g].size();
    if (n > R) { p.ok = false; break; }
    if (used + n > R) { ++p.last_tile; used = 0; }
    if (p.last_tile >= 4) { p.ok = false; break; }
    for (int q = 0; q < n; ++q) p.rows[p.last_tile * R + used + q] = grp[g][q];
    used += n;
    p.tile_of[g] = p.last_tile;
    p.end_of[g] = p.last_tile * R + used;
  }
  return p;
}
// degree-sorted, contiguous rows: a degree group may straddle tiles (lo < hi), its pass recomputes every tile it touches
struct Spanned {
  std::vector<int> rows, lo, hi, end_of;   // row -> unit; per group: first / last tile, exclusive end row
};
Spanned pack_contiguous(const Groups& grp, int R) {
  const int G = (int)grp.size();
  Spanned s{std::vector<int>(4 * R, -1), std::vector<int>(G), std::vector<int>(G), std::vector<int>(G)};
  int r = 0;
  for (int g = 0; g < G; ++g) {
    s.lo[g] = r / R;
    for (int j : grp[g]) s.rows[r++] = j;
    s.hi[g] = (r - 1) / R;
    s.end_of[g] = r;
  }
  return s;
}

// ---- [mt][ks]([hi | lo])[64 lanes][8] walk of a hidden H x H block for v_mfma_f32_32x32x16_bf16: element j of lane (c, h) is
// input row 16 ks + 8 (j >> 2) + 4 h + (j & 3) (the k order in which sf_bfrag hands registers 8 ks' .. 8 ks' + 7 of an accumulator
// tile to the MFMA).  parts = 1: single bf16 operands (srcB); parts = 2: split bf16, entry = logical index | part << 30, hi = bf16(w),
// lo = bf16(w - hi) (src16B of the NSF sampler image).  Returns the start of the block in dst.
int64_t bf16_walk(std::vector<int32_t>& dst, int parts, int HT, int nKS, const std::vector<int>& hrow_full, int64_t base, int H,
                  const Mask& mask) {
  const int64_t start = (int64_t)dst.size();
  for (int mt = 0; mt < HT; ++mt)
    for (int ks = 0; ks < nKS; ++ks)
      for (int part = 0; part < parts; ++part)
        for (int l = 0; l < 64; ++l)
          for (int j = 0; j < 8; ++j) {
            const int o = hrow_full[mt * 32 + (l & 31)];
            const int rho = 16 * ks + 8 * (j >> 2) + 4 * (l >> 5) + (j & 3);
            const int i = rho < 128 ? hrow_full[rho] : -1;
            const bool on = o >= 0 && i >= 0 && (!mask || mask(o, i));
            dst.push_back(on ? (int32_t)((base + (int64_t)o * H + i) | ((int64_t)part << 30)) : -1);
          }
  return start;
}

// ---- greedy LDS staging planner: whole items in execution order into at most four parts of at most `budget` bytes.  Item i is
// floats [cf[i], cf[i + 1]) of the fp32 image plus bf16 elements [cb[i], cb[i + 1]).  ok = 0: an item exceeds the budget or a fifth
// part would be needed (n and the offsets then stand where the planner stopped).
struct Parts {
  bool ok = true;
  int n = 0, off[5] = {0, 0, 0, 0, 0}, offB[5] = {0, 0, 0, 0, 0};
  std::vector<int> item_part;
};
Parts plan_parts(const std::vector<int>& cf, const std::vector<int>& cb, size_t budget) {
  Parts p;
  p.item_part.assign(cf.size() - 1, 0);
  auto bytes = [&](int f0, int b0, size_t i1) { return (size_t)(cf[i1] - f0) * 4 + (size_t)(cb[i1] - b0) * 2; };
  int f0 = 0, b0 = 0;   // start of the open part
  for (size_t i = 0; i + 1 < cf.size(); ++i) {
    if (bytes(cf[i], cb[i], i + 1) > budget) { p.ok = false; return p; }
    if (bytes(f0, b0, i + 1) > budget) {   // close the current part before this item
      if (p.n >= 3) { p.ok = false; return p; }
      ++p.n;
      p.off[p.n] = f0 = cf[i];
      p.offB[p.n] = b0 = cb[i];
    }
    p.item_part[i] = p.n;
  }
  ++p.n;
  p.off[p.n] = cf.back();
  p.offB[p.n] = cb.back();
  return p;
}

// ---- emitter of the cooperative 16-row training images (sf_layout.h: SfTrcDev, SfNscDev), one per transform: gather table
// srcC1 / srcC2, and for every logical parameter its place in the transform's gradient partial (gdstC) ----
struct CoopEmitter {
  struct At { int o; int64_t g; };   // where a block starts: in the transform's image, in its gradient partial
  SfLayout& L;
  int64_t tb;        // start of this transform in the image
  int64_t gbase;     // ... and of its gradient partial: t * g_stride.  g_stride is known only once transform 0 has been emitted;
                     // its entries are written with g_stride = 0, which is right because 0 * g_stride is 0 either way
  int64_t gcur = 0;  // cursor in the gradient partial

  // n_logical = end of this transform's logical parameter block
  CoopEmitter(SfLayout& L_, int t, int g_stride, int64_t n_logical) : L(L_) {
    while (L.srcC1.size() % 256) push(-1);
    tb = (int64_t)L.srcC1.size();
    gbase = (int64_t)t * g_stride;
    if (t == 0) L.gdstC.clear();
    if (L.gdstC.size() < (size_t)n_logical) L.gdstC.resize((size_t)n_logical, -1);
  }
  void push(int64_t a, int64_t b = -1) { L.srcC1.push_back((int32_t)a); L.srcC2.push_back((int32_t)b); }
  int here() const { return (int)((int64_t)L.srcC1.size() - tb); }
  At take(int64_t n_grad) { const At at{here(), gcur}; gcur += n_grad; return at; }
  void owns(int64_t idx, int64_t g) { L.gdstC[(size_t)idx] = (int32_t)(gbase + g); }
  // element (ro, ri) of a 16 x 16 gradient block: the accumulator of dW = delta . in^T as it stands
  static int64_t gpos(int ro, int ri) { return (ro & 3) * 64 + (ro >> 2) * 16 + ri; }

  At fwd(int OT, int IT, const WFn& fn) {   // forward block [ot][it][64 lanes][4]
    const At at = take((int64_t)OT * IT * 256);
    for (int ot = 0; ot < OT; ++ot)
      for (int it = 0; it < IT; ++it)
        for (int l = 0; l < 64; ++l)
          for (int r = 0; r < 4; ++r) {
            const int ro = l & 15, ri = 4 * (l >> 4) + r;
            const int64_t idx = fn(ot, ro, it, ri);
            push(idx);
            if (idx >= 0) owns(idx, at.g + ((int64_t)ot * IT + it) * 256 + gpos(ro, ri));
          }
    return at;
  }
  int tr(int ITr, int OTk, const WFn& fn) {   // transposed block: rows = forward input tiles, K = forward output tiles
    const int o = here();
    for (int it = 0; it < ITr; ++it)
      for (int ot = 0; ot < OTk; ++ot)
        for (int l = 0; l < 64; ++l)
          for (int r = 0; r < 4; ++r) push(fn(ot, 4 * (l >> 4) + r, it, l & 15));
    return o;
  }
  At bias(int OT, const BFn& f1, const BFn& f2 = nullptr) {   // bias block [ot][16], optionally the sum of two sources
    const At at = take((int64_t)OT * 16);
    for (int ot = 0; ot < OT; ++ot)
      for (int ro = 0; ro < 16; ++ro) {
        const int64_t a1 = f1(ot, ro), a2 = f2 ? f2(ot, ro) : -1;
        push(a1, a2);
        if (a1 >= 0) owns(a1, at.g + ot * 16 + ro);
        if (a2 >= 0) owns(a2, at.g + ot * 16 + ro);
      }
    return at;
  }
};

// ---- logical parameter offsets of one transform (the order of include/synference_hip.h) ----
struct MafT {
  int64_t W0, b0, Wc, bc, Wk[SF_NBMAX], bk[SF_NBMAX], Wf, bf;
  std::vector<int> sinv;   // physical slot -> logical dimension of this transform
  std::vector<int> urow;   // rows of the u tile
  std::vector<int> frow;   // rows of the final layer's output tile: (a, m) of slot p
};
struct NsfT {
  int64_t Win, bin, Wg[SF_NBMAX], bg[SF_NBMAX], W1[SF_NBMAX], b1[SF_NBMAX], W2[SF_NBMAX], b2[SF_NBMAX], Wout, bout;
  int64_t Lo = -1, Up = -1, Di = -1, Bi = -1;   // LU linear (D > 1)
  std::vector<int> idn;    // identity dimensions of this transform (the others are transformed)
  int d_id, d_tr, in_dim;
  std::vector<int> urow, crow;   // rows of the u tile / context groups: columns of Win
  std::vector<int> orow;         // spline head rows: [jp][pt][32]
};

// LU block: L[n][n] (strictly lower), U[n][n] (strictly upper), udiag[n], bias[n]; n = D in the flow images, 8 in the cooperative
// one.  emit(logical index or -1, offset in the cooperative gradient block: block 0 = dL, block 1 = dU, then 16 row sums: [0, 8)
// dbias, [8, 16) d udiag).
template <class Emit> void lu_block(const NsfT& l, int D, int n, Emit emit) {
  int cnt = 0;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) emit(j < i && i < D ? l.Lo + cnt++ : -1, CoopEmitter::gpos(i, j));
  cnt = 0;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) emit(j > i && j < D ? l.Up + cnt++ : -1, 256 + CoopEmitter::gpos(i, j));
  for (int i = 0; i < n; ++i) emit(D > 1 && i < D ? l.Di + i : -1, 512 + 8 + i);
  for (int i = 0; i < n; ++i) emit(D > 1 && i < D ? l.Bi + i : -1, 512 + i);
}

const char* desc_error(const sf_flow_desc& d) {
  if (d.kind != SF_MAF && d.kind != SF_NSF) return "kind must be SF_MAF or SF_NSF";
  if (d.D < 1 || d.D > SF_DMAX) return "D must be in 1..16";
  if (d.C < 1 || d.C > 512) return "C must be in 1..512";
  if (d.H < 1 || d.H > 128) return "H must be in 1..128";
  if (d.T < 1 || d.T > 64) return "T must be in 1..64";
  if (d.NB < 1 || d.NB > SF_NBMAX) return "NB must be in 1..4";
  if (d.kind == SF_NSF && (d.K < 2 || d.K > 16)) return "K must be in 2..16";
  if (!d.theta_mean || !d.theta_std || !d.x_mean || !d.x_std) return "z-score buffers must be given";
  return nullptr;
}

const size_t LDS_BUDGET = (size_t)152 * 1024;   // bytes of the 160 KiB LDS; the rest holds the persistent sampler's control block

struct LayoutBuilder {
  const sf_flow_desc& d;
  SfLayout& L;
  SfDev& v;
  const int D, C, H, T, NB, K;
  const bool maf;
  const Made made;
  int t = 0;   // the transform being emitted
  std::vector<int> hrow_full = std::vector<int>(4 * 32, -1);   // hidden physical row -> logical unit (32-row tiles)
  std::vector<int> h16row = std::vector<int>(4 * 16, -1);      // ... of the sampler's 16-row images
  std::vector<int> h16row_trc;  // rows of the cooperative training image: the placement without the skipped register (place_rows16)
  std::vector<int> hrow_out, hrow_in, crow_in;                 // hrow_full cut to HT tiles / nGh groups; context rows
  std::vector<std::vector<int>> sigma;                         // MAF physical slot maps
  std::vector<int32_t> gidx;
  Emitter E{L.src1, L.src2, &gidx};
  Emitter ET{L.srcT1, L.srcT2, nullptr};  // transposed image
  Emitter ES{L.src16a, L.src16b, nullptr};  // NSF sampler image, fp32 part (sf_layout.h, SfNsfSamp)
  int64_t P = 0;  // logical cursor

  LayoutBuilder(const sf_flow_desc& d_, SfLayout& L_)
      : d(d_), L(L_), v(L_.dev), D(d_.D), C(d_.C), H(d_.H), T(d_.T), NB(d_.NB), K(d_.K), maf(d_.kind == SF_MAF), made(d_.D) {}

  bool fail(const std::string& m) {
    L.error = m;
    return false;
  }
  // offsets are the same for every transform: recorded on the first one only
  void first(int& field, int64_t off) const { if (t == 0) field = (int)off; }
  void first(int& o, int& g, CoopEmitter::At at) const { if (t == 0) { o = at.o; g = (int)at.g; } }

  bool run() {
    init_descriptor();
    place_hidden_rows();
    if (!slot_maps()) return fail("perms is not a permutation");
    constants_image();
    for (t = 0; t < T; ++t) {
      if (maf) maf_transform();
      else nsf_transform();
    }
    close_images();
    if (!maf && L.nsfS.ok) close_nsf_sampler();
    close_images16();
    compact_image();
    if (!staging_plan()) return fail("hidden_bf16: one transform's fp32 + bf16 operand images must fit the 152 KiB LDS budget");
    close_coop();
    gradient_map();
    return true;
  }

  void init_descriptor() {
    std::memset(&v, 0, sizeof(v));
    std::memset(&L.trc, 0, sizeof(L.trc));
    std::memset(&L.nsc, 0, sizeof(L.nsc));
    std::memset(&L.nsfS, 0, sizeof(L.nsfS));
    v.kind = d.kind; v.D = D; v.C = C; v.H = H; v.T = T; v.K = K; v.NB = NB;
    v.scale_fn = d.scale_fn;
    v.HT = ceil_div(H, 32);
    v.nGu = ceil_div(D, 8);
    v.nGc = ceil_div(C, 8);
    v.nGh = ceil_div(H, 8);
    v.tail_bound = d.tail_bound; v.min_w = d.min_bin_width; v.min_h = d.min_bin_height;
    v.min_d = d.min_derivative; v.eps = d.maf_eps; v.lu_eps = d.lu_eps;
    v.inv_sqrt_h = (float)(1.0 / std::sqrt((double)H));
    v.deriv_const = (float)std::log(std::exp(1.0 - (double)d.min_derivative) - 1.0);
    v.hidden_bf16 = d.hidden_bf16 ? 1 : 0;
    if (!maf) {
      L.nsfS.ok = d.hidden_bf16 ? 0 : 1;
      v.PT = K <= 11 ? 2 : 3;  // PT=1 (K<=5) is not instantiated: K<=11 shares the 2-tile layout
      v.KMAX = (v.PT * 16 + 1) / 3;
      v.JP = ceil_div((D + 1) / 2, 2);
    }
  }

  // ---- hidden physical row -> logical unit ---------------------------------------------------
  // NSF: identity.  MAF: units sorted by MADE degree, every degree group kept inside one tile when
  // that fits in <= 4 tiles (then the masked HxH blocks are block-lower-triangular in tile/group
  // units and the autoregressive inverse can be evaluated incrementally).
  void place_hidden_rows() {
    if (maf) {
      Groups grp(made.mx);   // degree values mn .. mn + mx - 1; index g + mn of the descriptor's per-degree arrays (0 unused when mn == 1)
      for (int j = 0; j < H; ++j) grp[j % made.mx].push_back(j);
      place_rows32(grp);
      place_rows16(grp);
    } else {
      for (int j = 0; j < H; ++j) hrow_full[j] = j;
    }
    set_mt_kend();
    hrow_out.assign(hrow_full.begin(), hrow_full.begin() + v.HT * 32);
    hrow_in.assign(hrow_full.begin(), hrow_full.begin() + v.nGh * 8);
    crow_in = iota_rows(C, v.nGc * 8);
    v.nKS = ceil_div(v.nGh, 2);
  }

  // Aligned placement (one pass = one tile) costs extra tiles when the groups pack badly (H = 64, D = 8: 3 tiles
  // instead of 2, i.e. 1.5x the MFMA work of log_prob and training) and extra input groups, which can push the
  // transform's image out of the LDS.  Contiguous placement (a group may straddle tiles, its pass recomputes
  // every tile it touches) is taken instead when it saves a tile or is the only one of the two that fits the LDS.
  bool prefer_contiguous32(int ht_a, int ngh_a) const {
    auto image_floats = [&](int ht, int ngh) {
      return 256L * (ht * (v.nGu + v.nGc) + (long)NB * ht * ngh + ngh) + 64L * D * ht + 64L * (NB + 1) * ht;
    };
    const long lds_floats = (long)(LDS_BUDGET / 4);
    const int ht_c = ceil_div(H, 32), ngh_c = ceil_div(H, 8);
    return ht_a > ht_c || (image_floats(ht_a, ngh_a) > lds_floats && image_floats(ht_c, ngh_c) <= lds_floats);
  }
  void place_rows32(const Groups& grp) {
    const int G = (int)grp.size(), mn = made.mn;
    Packed a = pack_whole_groups(grp, 32, true);
    if (a.ok && D >= 2 && prefer_contiguous32(a.last_tile + 1, ceil_div(a.end_of[G - 1], 8))) a.ok = false;
    if (a.ok) {
      hrow_full = a.rows;
      v.HT = std::max(v.HT, a.last_tile + 1);
      for (int g = 0; g < G; ++g) {
        v.g_tile[g + mn] = v.g_lo[g + mn] = a.tile_of[g];
        v.g_kend[g + mn] = ceil_div(a.end_of[g], 8);
      }
      v.nGh = ceil_div(a.end_of[G - 1], 8);
    } else {
      const Spanned s = pack_contiguous(grp, 32);
      hrow_full = s.rows;
      for (int g = 0; g < G; ++g) {
        v.g_lo[g + mn] = s.lo[g];
        v.g_tile[g + mn] = s.hi[g];
        v.g_kend[g + mn] = ceil_div(s.end_of[g], 8);
      }
    }
    v.inc_ok = D >= 2 ? 1 : 0;
  }

  // 16-row tiles for the 16x16x4 incremental inverse: whole degree groups, at most 4 tiles; else (H <= 64) contiguous
  void place_rows16(const Groups& grp) {
    const int G = (int)grp.size(), mn = made.mn;
    const Packed p = pack_whole_groups(grp, 16, D >= 2 && NB <= 2);
    h16row = p.rows;
    for (int g = 0; g < G; ++g) v.g16_tile[g + mn] = v.g16_lo[g + mn] = p.tile_of[g];
    h16row_trc = h16row;
    bool ok16 = p.ok;
    int tiles = p.last_tile + 1;
    if (ok16) {
      skip_register3(grp, p);
    } else if (D >= 2 && NB <= 2 && H <= 64) {
      // whole groups do not fit four tiles: pack the degree-sorted units contiguously; a group may then straddle
      // tiles and its pass recomputes every tile it touches (sf_pass16_span)
      const Spanned s = pack_contiguous(grp, 16);
      h16row = h16row_trc = s.rows;
      for (int g = 0; g < G; ++g) { v.g16_lo[g + mn] = s.lo[g]; v.g16_tile[g + mn] = s.hi[g]; }
      tiles = (H - 1) / 16 + 1;
      ok16 = true;
      v.m16_span = 1;
    }
    v.m16_ok = ok16 ? 1 : 0;
    v.nT16 = ok16 ? tiles : 0;
    v.nC16 = ceil_div(C, 16);
  }
  // One degree group per tile with D = 3..5 (the shapes of the unrolled kernels, sf_maf16_seq_d): a group of n <= 12 units
  // leaves register 3 of every row group empty -- unit q sits in row 4 (q / KS) + q % KS, KS = max(3, ceil(n / 4)) -- so
  // that the fourth k-step of every MFMA that reads the tile (rows 3, 7, 11, 15: sf_mma16) and the fourth tanh register
  // are structural zeros, which the fused passes skip (sf_pass16g).  Groups of 13..16 units keep their rows (KS = 4).
  // Every block of the sampler's 16-row images is laid out through h16row -- part A, the fp32 and split-bf16 hidden blocks,
  // the head tile, W' (k_maf_fuse16 reads the image), the compact image, the context-table weights -- so they all follow;
  // kernels that keep four k-steps multiply zeros as before.  The cooperative training image (sf_trainc.hip) keeps the rows
  // 0 .. n - 1 (h16row_trc): another placement would reorder the sums of its MFMAs, and a fit of thousands of steps
  // amplifies that rounding into other weights -- training must not depend on a sampler optimisation.
  // m16_k3 = trailing tiles with KS = 3 (degrees are dealt as j % (D - 1): the larger groups come first).
  void skip_register3(const Groups& grp, const Packed& p) {
    const int G = (int)grp.size();
    if (D < 3 || D > 5 || p.last_tile + 1 != D - 1) return;
    for (int g = 0; g < G; ++g)
      if (p.tile_of[g] != g) return;   // (not one group per tile)
    std::vector<int> ks(G);
    for (int g = 0; g < G; ++g) {
      const int n = (int)grp[g].size();
      ks[g] = std::max(3, ceil_div(n, 4));
      for (int r = 0; r < 16; ++r) h16row[g * 16 + r] = -1;
      for (int q = 0; q < n; ++q) h16row[g * 16 + 4 * (q / ks[g]) + q % ks[g]] = grp[g][q];
    }
    while (v.m16_k3 < G && ks[G - 1 - v.m16_k3] == 3) ++v.m16_k3;
  }

  // input groups needed by hidden output tile mt: those that cover every degree group with rows in mt
  void set_mt_kend() {
    for (int mt = 0; mt < 4; ++mt) v.mt_kend[mt] = v.nGh;
    if (!maf || !v.inc_ok) return;
    for (int mt = 0; mt < 4; ++mt) {
      int k = 0;
      for (int g = made.mn; g < made.mn + made.mx; ++g)
        if (v.g_lo[g] <= mt && mt <= v.g_tile[g]) k = std::max(k, v.g_kend[g]);
      if (k > 0) v.mt_kend[mt] = k;
    }
  }

  // ---- MAF physical slot maps: sigma_T = identity, sigma_t = sigma_{t+1} o perm_t^{-1} ----
  bool slot_maps() {
    sigma.assign(T + 1, std::vector<int>(D));
    for (int tt = 0; tt <= T; ++tt)
      for (int i = 0; i < D; ++i) sigma[tt][i] = i;
    if (!maf) return true;
    for (int tt = T - 1; tt >= 0; --tt) {
      std::vector<int> perm(D);
      for (int j = 0; j < D; ++j) perm[j] = d.perms ? d.perms[tt * D + j] : j;
      std::vector<char> seen(D, 0);
      for (int j = 0; j < D; ++j) {
        if (perm[j] < 0 || perm[j] >= D || seen[perm[j]]) return false;
        seen[perm[j]] = 1;
      }
      // logical j of transform t+1 input  <-  logical perm[j] of transform t output
      for (int j = 0; j < D; ++j) sigma[tt][perm[j]] = sigma[tt + 1][j];
    }
    return true;
  }

  void constants_image() {
    std::vector<int> tdim(D);  // phys slot p holds logical theta dim tdim[p]
    for (int i = 0; i < D; ++i) tdim[sigma[0][i]] = i;
    v.c_pscale = 0; v.c_pshift = SF_DMAX; v.c_tdim = 2 * SF_DMAX;
    v.c_xmean = 3 * SF_DMAX; v.c_xstd = 3 * SF_DMAX + ((C + 3) / 4) * 4;
    L.cst.assign(v.c_xstd + ((C + 3) / 4) * 4, 0.f);
    double ld0 = 0;
    for (int p = 0; p < D; ++p) {
      float sd = d.theta_std[tdim[p]], mu = d.theta_mean[tdim[p]];
      float sc = 1.0f / sd;
      L.cst[v.c_pscale + p] = sc;
      L.cst[v.c_pshift + p] = -mu / sd;
      L.cst[v.c_tdim + p] = (float)tdim[p];
      ld0 += std::log(std::fabs((double)sc));
    }
    v.logdet0 = (float)ld0;
    for (int i = 0; i < C; ++i) {
      L.cst[v.c_xmean + i] = d.x_mean[i];
      L.cst[v.c_xstd + i] = d.x_std[i];
    }
    for (int i = C; i < ((C + 3) / 4) * 4; ++i) L.cst[v.c_xstd + i] = 1.f;
    v.c_dslot = (int)L.cst.size();
    L.cst.resize(L.cst.size() + (size_t)T * SF_DMAX, 0.f);
    for (int tt = 0; tt < T; ++tt)
      for (int i = 0; i < D; ++i) L.cst[v.c_dslot + tt * SF_DMAX + i] = (float)sigma[tt][i];  // degree i+1
  }

  // bf16 image of one transform's hidden blocks (hidden_bf16; srcB): opened once per transform, then one block per call
  void bf16_open() {
    while (L.srcB.size() % 64) L.srcB.push_back(-1);
    if (t == 1) v.tB_stride = (int)L.srcB.size();
  }
  int64_t emit_bf16(int64_t base, const Mask& mask) {
    while (L.srcB.size() % 8) L.srcB.push_back(-1);
    return bf16_walk(L.srcB, 1, v.HT, v.nKS, hrow_full, base, H, mask);
  }

  // =========================================== MAF ===========================================
  void maf_transform() {
    MafT m;
    m.W0 = P; m.b0 = m.W0 + (int64_t)H * D; m.Wc = m.b0 + H; m.bc = m.Wc + (int64_t)H * C;
    int64_t cur = m.bc + H;
    for (int k = 0; k < NB; ++k) { m.Wk[k] = cur; m.bk[k] = cur + (int64_t)H * H; cur = m.bk[k] + H; }
    m.Wf = cur; m.bf = m.Wf + (int64_t)2 * D * H;
    P = m.bf + 2 * D;
    m.sinv.resize(D);
    for (int i = 0; i < D; ++i) m.sinv[sigma[t][i]] = i;
    m.urow.assign(v.nGu * 8, -1);
    for (int p = 0; p < D; ++p) m.urow[p] = m.sinv[p];
    m.frow.assign(32, -1);
    for (int p = 0; p < D; ++p) {
      m.frow[sf_tile_row(2 * (p >> 1), p & 1)] = 2 * m.sinv[p];
      m.frow[sf_tile_row(2 * (p >> 1) + 1, p & 1)] = 2 * m.sinv[p] + 1;
    }
    maf_forward(m);
    maf_transposed(m);
    if (v.m16_ok) {
      maf_image16(m);
      maf_split16(m);
    }
    if (v.m16_ok && NB == 2 && D <= 8) maf_coop(m);
  }

  void maf_forward(const MafT& m) {
    const int HT = v.HT;
    const int64_t tb = E.pad_to(64);
    if (t == 1) v.t_stride = (int)tb;
    first(v.o_w0, E.linear(HT, v.nGu, hrow_out, m.urow, m.W0, D, 1, made.mask(&Made::in)) - tb);
    first(v.o_wc, E.linear(HT, v.nGc, hrow_out, crow_in, m.Wc, C, 1, nullptr) - tb);
    first(v.o_b0, E.bias(HT, hrow_out, m.b0, m.bc) - tb);
    for (int k = 0; k < NB; ++k) {
      first(v.o_wk[k], E.linear(HT, v.nGh, hrow_out, hrow_in, m.Wk[k], H, 1, made.mask(&Made::hid)) - tb);
      first(v.o_bk[k], E.bias(HT, hrow_out, m.bk[k], -1) - tb);
    }
    first(v.o_wf, E.linear(1, v.nGh, m.frow, hrow_in, m.Wf, H, 1, made.mask(&Made::head)) - tb);
    first(v.o_bf, E.bias(1, m.frow, m.bf, -1) - tb);
    // head rows once more, laid out for a per-lane dot product (incremental inverse): for physical
    // slot q the (a, m) rows, split by row half h, indexed like the lane's activation registers
    first(v.o_hv, E.pad_to(4) - tb);
    for (int q = 0; q < D; ++q)
      for (int ab = 0; ab < 2; ++ab)
        for (int h = 0; h < 2; ++h)
          for (int mt = 0; mt < HT; ++mt)
            for (int r = 0; r < 16; ++r) {
              const int unit = hrow_full[mt * 32 + sf_tile_row(r, h)];
              const int orow_l = 2 * m.sinv[q] + ab;
              const bool on = unit >= 0 && made.head(orow_l, unit);
              E.push(on ? (int32_t)(m.Wf + (int64_t)orow_l * H + unit) : -1, -1);
            }
    first(v.o_hvb, E.pad_to(4) - tb);
    for (int q = 0; q < D; ++q)
      for (int ab = 0; ab < 2; ++ab) E.push((int32_t)(m.bf + 2 * m.sinv[q] + ab), -1);
    if (v.hidden_bf16) {
      bf16_open();
      for (int k = 0; k < NB; ++k) first(v.oB_wk[k], emit_bf16(m.Wk[k], made.mask(&Made::hid)));
    }
  }

  // transposed operands for the data-gradient pass: delta_in = W^T delta_out.  A block's row is the forward INPUT index, its
  // column the forward OUTPUT index: W[i][o] at base + o + i * in_dim
  void maf_transposed(const MafT& m) {
    const int HT = v.HT;
    const int64_t tbT = ET.pad_to(64);
    if (t == 1) v.tT_stride = (int)tbT;
    v.nGf = ceil_div(2 * ((D + 1) / 2), 4);
    std::vector<int> urow32(32, -1);
    for (int p = 0; p < D; ++p) urow32[p] = m.sinv[p];
    first(v.oT_wf, ET.linear(HT, v.nGf, hrow_out, m.frow, m.Wf, 1, H, made.maskT(&Made::head)) - tbT);
    for (int k = 0; k < NB; ++k)
      first(v.oT_wk[k], ET.linear(HT, v.nGh, hrow_out, hrow_in, m.Wk[k], 1, H, made.maskT(&Made::hid)) - tbT);
    first(v.oT_w0, ET.linear(1, v.nGh, urow32, hrow_in, m.W0, 1, D, made.maskT(&Made::in)) - tbT);
    const int CT = ceil_div(C, 32);
    first(v.oT_wc, ET.linear(CT, v.nGh, iota_rows(C, CT * 32), hrow_in, m.Wc, 1, C, nullptr) - tbT);
  }

  // ---- 16-row-granular image for the incremental inverse ------------------------------------
  void maf_image16(const MafT& m) {
    auto push16 = [&](int32_t a, int32_t b) { L.src16a.push_back(a); L.src16b.push_back(b); };
    auto pad16 = [&](size_t q) { while (L.src16a.size() % q) push16(-1, -1); };
    pad16(1024);  // whole 4 KiB groups: the staging loop copies 4 x 1 KiB per address
    const int64_t tb16 = (int64_t)L.src16a.size();
    if (t == 1) v.t16_stride = (int)tb16;
    auto here = [&]() { return (int64_t)L.src16a.size() - tb16; };
    // weight block [ot][it][64 lanes][4]: lane l: out row ot*16+(l&15), in rows it*16 + 4*(l>>4) + r
    // second index SF_PACK_TANH_SCALE (-2): the packed value is multiplied by 2 log2(e) -- the hidden blocks' weights and
    // biases of the 16-row images carry the factor of tanh(x) = 1 - 2 / (1 + 2^(2 log2(e) x)), so that the kernels'
    // tanh starts at the exp2 (the kernel is bound by vector issue: one multiply per activation less)
    auto linear16 = [&](int OT, int IT, const std::vector<int>& orow, const std::vector<int>& irow, int64_t base,
                        int in_dim, const Mask& mask, int32_t second = -1) {
      for (int ot = 0; ot < OT; ++ot)
        for (int it = 0; it < IT; ++it)
          for (int l = 0; l < 64; ++l)
            for (int r = 0; r < 4; ++r) {
              const int oo = orow[ot * 16 + (l & 15)], ii = irow[it * 16 + 4 * (l >> 4) + r];
              const bool on = oo >= 0 && ii >= 0 && (!mask || mask(oo, ii));
              push16(on ? (int32_t)(base + (int64_t)oo * in_dim + ii) : -1, on ? second : -1);
            }
    };
    auto bias16 = [&](int OT, const std::vector<int>& orow, int64_t b1, int64_t b2) {
      for (int ot = 0; ot < OT; ++ot)
        for (int g4 = 0; g4 < 4; ++g4)
          for (int r = 0; r < 4; ++r) {
            const int oo = orow[ot * 16 + 4 * g4 + r];
            push16(oo >= 0 ? (int32_t)(b1 + oo) : -1,
                   oo < 0 ? -1 : (b2 >= 0 ? (int32_t)(b2 + oo) : (b2 == SF_PACK_TANH_SCALE ? SF_PACK_TANH_SCALE : -1)));
          }
    };
    std::vector<int> u16(16, -1);
    for (int p = 0; p < D; ++p) u16[p] = m.sinv[p];
    const std::vector<int> c16 = iota_rows(C, v.nC16 * 16);
    const int NT = v.nT16;
    // part A (everything but the hidden H x H blocks; staged by both sampler kernels)
    first(v.o16_w0, here());
    linear16(NT, 1, h16row, u16, m.W0, D, made.mask(&Made::in));
    first(v.o16_b0, here());
    bias16(NT, h16row, m.b0, m.bc);
    for (int k = 0; k < NB && k < 2; ++k) {
      first(v.o16_bk[k], here());
      bias16(NT, h16row, m.bk[k], SF_PACK_TANH_SCALE);
    }
    // head rows for the per-lane dot product: [slot][g4][tile (4)][r][a|m]  (a and m interleaved: one packed
    // v_pk_fma_f32 updates both partial sums)
    first(v.o16_hv, here());
    for (int q = 0; q < D; ++q)
      for (int g4 = 0; g4 < 4; ++g4)
        for (int tl = 0; tl < 4; ++tl)
          for (int r = 0; r < 4; ++r)
            for (int ab = 0; ab < 2; ++ab) {
              const int unit = tl < NT ? h16row[tl * 16 + 4 * g4 + r] : -1;
              const int orow_l = 2 * m.sinv[q] + ab;
              const bool on = unit >= 0 && made.head(orow_l, unit);
              push16(on ? (int32_t)(m.Wf + (int64_t)orow_l * H + unit) : -1, -1);
            }
    first(v.o16_hvb, here());
    for (int q = 0; q < D; ++q)
      for (int ab = 0; ab < 2; ++ab) push16((int32_t)(m.bf + 2 * m.sinv[q] + ab), -1);
    // the same head rows as ONE 16-row output tile of the matrix pipe (D <= 8): row 2q + ab = (a | m) of physical
    // slot q, one A fragment per hidden tile, and the head biases as that tile's initial accumulator
    if (D <= 8) {
      pad16(4);
      first(v.o16_wh, here());
      std::vector<int> hrow16(16, -1);
      for (int q = 0; q < D; ++q)
        for (int ab = 0; ab < 2; ++ab) hrow16[2 * q + ab] = 2 * m.sinv[q] + ab;
      linear16(1, NT, hrow16, h16row, m.Wf, H, made.mask(&Made::head));
      first(v.o16_bh, here());
      bias16(1, hrow16, m.bf, -1);
      pad16(4);
      first(v.o16_wp, here());
      for (int i = 0; i < NT * 256; ++i) push16(-1, -1);   // (computed on the device: k_maf_fuse16)
    } else if (t == 0) {
      v.o16_wh = v.o16_bh = -1;
      v.o16_wp = -1;
    }
    // what the sampler stages when the per-galaxy context table exists (it then never reads Wc) ends here
    pad16(1024);
    first(v.t16_a_tab, here());
    first(v.o16_wc, here());
    linear16(NT, v.nC16, h16row, c16, m.Wc, C, nullptr);
    pad16(1024);
    first(v.t16_a, here());
    // part B: the hidden blocks in fp32 (k_maf_inv16: parity hook, acceptance counts, explicit rounds)
    for (int k = 0; k < NB && k < 2; ++k) {
      first(v.o16_wk[k], here());
      linear16(NT, NT, h16row, h16row, m.Wk[k], H, made.mask(&Made::hid), SF_PACK_TANH_SCALE);
    }
  }

  // ---- split-bf16 image of the hidden blocks (k_maf_samp16): per block [ot][pair][hi|lo][64 lanes][8 bf16];
  // element j of lane l is W[out row ot*16 + (l&15)][in row 16*(2*pair + (j>>2)) + 4*(l>>4) + (j&3)] -- the k order
  // in which two 16-row activation tiles (4 registers each, lane = sample + 16 * row group) form the B operand
  // of v_mfma_f32_16x16x32_bf16 without moving between lanes.  hi = bf16(w), lo = bf16(w - hi): three products
  // hi.hi + hi.lo + lo.hi reproduce the fp32 product to ~2^-17 relative.
  void maf_split16(const MafT& m) {
    while (L.src16B.size() % 2048) L.src16B.push_back(-1);  // whole 4 KiB groups (2 bf16 per 32-bit word)
    const int64_t tbB = (int64_t)L.src16B.size();
    if (t == 1) v.t16B_stride = (int)(tbB / 2);
    const int NT = v.nT16, NP = (NT + 1) / 2;
    v.nP16 = NP;
    for (int k = 0; k < NB && k < 2; ++k) {
      first(v.o16B_wk[k], ((int64_t)L.src16B.size() - tbB) / 2);
      for (int ot = 0; ot < NT; ++ot)
        for (int pr = 0; pr < NP; ++pr) {
          // aligned placement: tiles above `ot` hold strictly higher degrees, so pairs above ot's own are all
          // masked and are not stored (entry index ot + (ot == 3) + pr); 36 KB instead of 44 KB per transform for
          // four tiles = a fourth workgroup per CU.  Contiguous placement keeps every pair.
          if (!v.m16_span && pr > ot / 2) continue;
          for (int part = 0; part < 2; ++part)
            for (int l = 0; l < 64; ++l)
              for (int j = 0; j < 8; ++j) {
                const int it = 2 * pr + (j >> 2);
                const int oo = h16row[ot * 16 + (l & 15)];
                const int ii = it < NT ? h16row[it * 16 + 4 * (l >> 4) + (j & 3)] : -1;
                const bool on = oo >= 0 && ii >= 0 && made.hid(oo, ii);
                L.src16B.push_back(on ? (int32_t)((m.Wk[k] + (int64_t)oo * H + ii) | ((int64_t)part << 30) | SF_PACK_SPLIT_SCALED) : -1);
              }
        }
    }
  }

  // ---- cooperative 16-row training image (sf_layout.h, SfTrcDev; sf_trainc.hip) -------------------------
  // rows of the input tiles and the unmasked hidden blocks: the same for every transform, kept in the constants image
  void maf_coop_setup() {
    SfTrcDev& c = L.trc;
    const int NT = v.nT16;
    c.ok = 1;
    c.NT = NT;
    // rows of the input tiles: slot rows first (fixed), context features fill what is left
    std::vector<int> insrc(16, -1);
    int f = 0;
    for (int rho = 0; rho < 16 && f < C; ++rho) {
      const bool slot_row = (rho & 3) < 2 && 2 * (rho >> 2) + (rho & 3) < D;
      if (!slot_row) insrc[rho] = f++;
    }
    while (f < C) {
      for (int rho = 0; rho < 16; ++rho) insrc.push_back(f < C ? f++ : -1);
    }
    c.NI = (int)insrc.size() / 16;
    c.c_insrc = (int)L.cst.size();
    for (int q : insrc) L.cst.push_back((float)q);
    // unmasked hidden blocks and the tile bounds they imply
    for (int ot = 0; ot < 4; ++ot) { c.kend[ot] = 0; c.kbeg[ot] = NT > 0 ? NT - 1 : 0; }
    c.c_jobs = (int)L.cst.size();
    c.n_jobs = 0;
    for (int ot = 0; ot < NT; ++ot)
      for (int it = 0; it < NT; ++it) {
        bool any = false;
        for (int ro = 0; ro < 16 && !any; ++ro)
          for (int ri = 0; ri < 16 && !any; ++ri) {
            const int oo = h16row_trc[ot * 16 + ro], ii = h16row_trc[it * 16 + ri];
            any = oo >= 0 && ii >= 0 && made.hid(oo, ii);
          }
        if (any) {
          c.kend[ot] = std::max(c.kend[ot], it);
          c.kbeg[it] = std::min(c.kbeg[it], ot);
          L.cst.push_back((float)(ot * 4 + it));
          ++c.n_jobs;
        }
      }
    while (L.cst.size() % 4) L.cst.push_back(0.f);
  }
  void maf_coop(const MafT& m) {
    SfTrcDev& c = L.trc;
    if (t == 0) maf_coop_setup();
    const int NT = c.NT, NI = c.NI;
    CoopEmitter ce(L, t, c.g_stride, P);
    if (t == 1) c.t_stride = (int)ce.tb;
    const std::vector<int>& hrow = h16row_trc;
    // logical index of W[(to, ro)][(ti, ri)] for every layer, -1 = structural zero
    auto w_in = [&](int to, int ro, int ti, int ri) -> int64_t {
      const int oo = hrow[to * 16 + ro];
      if (oo < 0) return -1;
      if (ti == 0 && (ri & 3) < 2) {
        const int p = 2 * (ri >> 2) + (ri & 3);
        if (p < D) return made.in(oo, m.sinv[p]) ? m.W0 + (int64_t)oo * D + m.sinv[p] : -1;
      }
      const int fsrc = (int)L.cst[c.c_insrc + ti * 16 + ri];
      return fsrc >= 0 ? m.Wc + (int64_t)oo * C + fsrc : -1;
    };
    auto w_hid = [&](int64_t base) -> WFn {
      return [&, base](int to, int ro, int ti, int ri) -> int64_t {
        const int oo = hrow[to * 16 + ro], ii = hrow[ti * 16 + ri];
        return (oo >= 0 && ii >= 0 && made.hid(oo, ii)) ? base + (int64_t)oo * H + ii : -1;
      };
    };
    auto head_row = [&](int ro) -> int {  // logical output row of head-tile row ro, -1 = padding
      const int p = 2 * (ro >> 2) + (ro & 1);
      if (p >= D) return -1;
      return 2 * m.sinv[p] + ((ro & 3) >= 2 ? 1 : 0);
    };
    auto w_head = [&](int /*to*/, int ro, int ti, int ri) -> int64_t {
      const int orow_l = head_row(ro), ii = hrow[ti * 16 + ri];
      return (orow_l >= 0 && ii >= 0 && made.head(orow_l, ii)) ? m.Wf + (int64_t)orow_l * H + ii : -1;
    };
    auto hid_bias = [&](int64_t base) -> BFn {
      return [&, base](int ot, int ro) -> int64_t { const int oo = hrow[ot * 16 + ro]; return oo >= 0 ? base + oo : -1; };
    };
    auto head_bias = [&](int, int ro) -> int64_t { const int r_ = head_row(ro); return r_ >= 0 ? m.bf + r_ : -1; };
    // forward blocks
    first(c.o_win, c.g_win, ce.fwd(NT, NI, w_in));
    first(c.o_b0, c.g_b0, ce.bias(NT, hid_bias(m.b0), hid_bias(m.bc)));
    first(c.o_w1, c.g_w1, ce.fwd(NT, NT, w_hid(m.Wk[0])));
    first(c.o_b1, c.g_b1, ce.bias(NT, hid_bias(m.bk[0])));
    first(c.o_w2, c.g_w2, ce.fwd(NT, NT, w_hid(m.Wk[1])));
    first(c.o_b2, c.g_b2, ce.bias(NT, hid_bias(m.bk[1])));
    first(c.o_wf, c.g_wf, ce.fwd(1, NT, w_head));
    first(c.o_bf, c.g_bf, ce.bias(1, head_bias));
    // transposed blocks (data gradients)
    first(c.o_wfT, ce.tr(NT, 1, w_head));
    first(c.o_w2T, ce.tr(NT, NT, w_hid(m.Wk[1])));
    first(c.o_w1T, ce.tr(NT, NT, w_hid(m.Wk[0])));
    first(c.o_winT, ce.tr(NI, NT, w_in));
    if (t == 0) c.g_stride = (int)((ce.gcur + 63) / 64 * 64);
  }

  // =========================================== NSF ===========================================
  void nsf_transform() {
    NsfT n;
    const int NP = 3 * K - 1;
    for (int i = 0; i < D; ++i)
      if ((i % 2) != (t % 2)) n.idn.push_back(i);
    n.d_id = (int)n.idn.size(); n.d_tr = D - n.d_id;
    n.in_dim = n.d_id + C;
    n.Win = P; n.bin = n.Win + (int64_t)H * n.in_dim;
    int64_t cur = n.bin + H;
    for (int k = 0; k < NB; ++k) {
      n.Wg[k] = cur; n.bg[k] = n.Wg[k] + (int64_t)H * C;
      n.W1[k] = n.bg[k] + H; n.b1[k] = n.W1[k] + (int64_t)H * H;
      n.W2[k] = n.b1[k] + H; n.b2[k] = n.W2[k] + (int64_t)H * H;
      cur = n.b2[k] + H;
    }
    n.Wout = cur; n.bout = n.Wout + (int64_t)n.d_tr * NP * H;
    cur = n.bout + (int64_t)n.d_tr * NP;
    if (D > 1) {
      const int nl = D * (D - 1) / 2;
      n.Lo = cur; n.Up = n.Lo + nl; n.Di = n.Up + nl; n.Bi = n.Di + D;
      cur = n.Bi + D;
    }
    P = cur;
    n.urow.assign(v.nGu * 8, -1);  // u tile row = phys slot = logical dim
    for (int j = 0; j < n.d_id; ++j) n.urow[n.idn[j]] = j;
    n.crow.assign(v.nGc * 8, -1);
    for (int i = 0; i < C; ++i) n.crow[i] = n.d_id + i;
    // spline head rows: [jp][pt][32]
    n.orow.assign(v.JP * v.PT * 32, -1);
    for (int jp = 0; jp < v.JP; ++jp)
      for (int pt = 0; pt < v.PT; ++pt)
        for (int rho = 0; rho < 32; ++rho) {
          int h = (rho >> 2) & 1, r = (rho & 3) + 4 * (rho >> 3);
          int s = pt * 16 + r, kdim = 2 * jp + h, row = -1;
          if (kdim < n.d_tr) {
            if (s < v.KMAX) { if (s < K) row = kdim * NP + s; }
            else if (s < 2 * v.KMAX) { if (s - v.KMAX < K) row = kdim * NP + K + (s - v.KMAX); }
            else if (s < 3 * v.KMAX - 1) { if (s - 2 * v.KMAX < K - 1) row = kdim * NP + 2 * K + (s - 2 * v.KMAX); }
          }
          n.orow[(jp * v.PT + pt) * 32 + rho] = row;
        }
    nsf_fp32<true>(E, v, n);
    if (v.hidden_bf16) {
      bf16_open();
      for (int k = 0; k < NB; ++k) {
        first(v.oB_w1[k], emit_bf16(n.W1[k], nullptr));
        first(v.oB_w2[k], emit_bf16(n.W2[k], nullptr));
      }
    }
    if (L.nsfS.ok) {   // sampler image: the same blocks without W1 / W2, and those as split bf16
      nsf_fp32<false>(ES, L.nsfS, n);
      nsf_split(n);
    }
    nsf_transposed(n);
    if (NB == 2 && D >= 2 && D <= 8 && H <= 80 && 3 * K - 1 <= 32 && 8 + C <= 48) nsf_coop(n);
  }

  // the fp32 blocks of one transform, into the main image (HIDDEN: SfDev) or the sampler image (no W1 / W2 blocks: SfNsfSamp)
  template <bool HIDDEN, class Dst> void nsf_fp32(Emitter& Em, Dst& o, const NsfT& n) {
    const int HT = v.HT;
    const int64_t tb = Em.pad_to(64);
    if (t == 1) o.t_stride = (int)tb;
    first(o.o_winu, Em.linear(HT, v.nGu, hrow_out, n.urow, n.Win, n.in_dim, 1, nullptr) - tb);
    first(o.o_winc, Em.linear(HT, v.nGc, hrow_out, n.crow, n.Win, n.in_dim, 1, nullptr) - tb);
    first(o.o_bin, Em.bias(HT, hrow_out, n.bin, -1) - tb);
    for (int k = 0; k < NB; ++k) {
      first(o.o_wg[k], Em.linear(HT, v.nGc, hrow_out, crow_in, n.Wg[k], C, 1, nullptr) - tb);
      first(o.o_bg[k], Em.bias(HT, hrow_out, n.bg[k], -1) - tb);
      if constexpr (HIDDEN) first(o.o_w1[k], Em.linear(HT, v.nGh, hrow_out, hrow_in, n.W1[k], H, 1, nullptr) - tb);
      first(o.o_b1[k], Em.bias(HT, hrow_out, n.b1[k], -1) - tb);
      if constexpr (HIDDEN) first(o.o_w2[k], Em.linear(HT, v.nGh, hrow_out, hrow_in, n.W2[k], H, 1, nullptr) - tb);
      first(o.o_b2[k], Em.bias(HT, hrow_out, n.b2[k], -1) - tb);
    }
    first(o.o_wout, Em.linear(v.JP * v.PT, v.nGh, n.orow, hrow_in, n.Wout, H, 1, nullptr) - tb);
    first(o.o_bout, Em.bias(v.JP * v.PT, n.orow, n.bout, -1) - tb);
    first(o.o_lu, Em.pad_to(4) - tb);
    lu_block(n, D, D, [&](int64_t idx, int64_t) { Em.push((int32_t)idx, -1); });
  }

  // split-bf16 hidden blocks of the sampler image (bf16_walk, two parts)
  void nsf_split(const NsfT& n) {
    SfNsfSamp& sS = L.nsfS;
    while (L.src16B.size() % 64) L.src16B.push_back(-1);
    if (t == 1) sS.tB_stride = (int)L.src16B.size();
    for (int k = 0; k < NB; ++k) {
      first(sS.oB_w1[k], bf16_walk(L.src16B, 2, v.HT, v.nKS, hrow_full, n.W1[k], H, nullptr));
      first(sS.oB_w2[k], bf16_walk(L.src16B, 2, v.HT, v.nKS, hrow_full, n.W2[k], H, nullptr));
    }
  }

  // transposed operands for the data-gradient pass (row = forward input, column = forward output)
  void nsf_transposed(const NsfT& n) {
    const int HT = v.HT;
    const int64_t tbT = ET.pad_to(64);
    if (t == 1) v.tT_stride = (int)tbT;
    for (int jp = 0; jp < v.JP; ++jp) {
      std::vector<int> qrow(n.orow.begin() + jp * v.PT * 32, n.orow.begin() + (jp + 1) * v.PT * 32);
      const int64_t o = ET.linear(HT, v.PT * 4, hrow_out, qrow, n.Wout, 1, H, nullptr) - tbT;
      if (jp == 0) first(v.oT_wout, o);
    }
    for (int k = 0; k < NB; ++k) {
      first(v.oT_w2[k], ET.linear(HT, v.nGh, hrow_out, hrow_in, n.W2[k], 1, H, nullptr) - tbT);
      first(v.oT_w1[k], ET.linear(HT, v.nGh, hrow_out, hrow_in, n.W1[k], 1, H, nullptr) - tbT);
    }
    std::vector<int> urow32(32, -1);
    for (int j = 0; j < n.d_id; ++j) urow32[n.idn[j]] = j;
    first(v.oT_winu, ET.linear(1, v.nGh, urow32, hrow_in, n.Win, 1, n.in_dim, nullptr) - tbT);
    const int CT = ceil_div(C, 32);
    std::vector<int> crow32(CT * 32, -1);
    for (int i = 0; i < C; ++i) crow32[i] = n.d_id + i;
    first(v.oT_wc, ET.linear(CT, v.nGh, crow32, hrow_in, n.Win, 1, n.in_dim, nullptr) - tbT);
    for (int k = 0; k < NB; ++k)
      first(v.oT_wg[k], ET.linear(CT, v.nGh, iota_rows(C, CT * 32), hrow_in, n.Wg[k], 1, C, nullptr) - tbT);
  }

  // ---- cooperative 16-row training image (sf_layout.h, SfNscDev; sf_nsfc.hip) -----------------------------
  void nsf_coop(const NsfT& n) {
    SfNscDev& c = L.nsc;
    const int NP = 3 * K - 1;
    const int NT = ceil_div(H, 16), NI = ceil_div(8 + C, 16);
    const int OTQ = NP <= 24 ? 6 : 8, KM = OTQ == 6 ? 8 : 11;
    if (t == 0) {
      c.ok = 1;
      c.NT = NT; c.NI = NI; c.OTQ = OTQ; c.KM = KM;
      c.kc_h = ceil_div(H - 16 * (NT - 1), 4);
      c.kc_in[0] = 4; c.kc_in[1] = c.kc_in[2] = 0;
      for (int it = 1; it < NI; ++it) c.kc_in[it] = ceil_div(std::min(16, C - 8 - 16 * (it - 1)), 4);
    }
    CoopEmitter ce(L, t, c.g_stride, P);
    if (t == 1) c.t_stride = (int)ce.tb;
    // row maps (sf_layout.h)
    auto hid_unit = [&](int tile, int rho) -> int { const int u = tile * 16 + (rho >> 2) + 4 * (rho & 3); return u < H ? u : -1; };
    std::vector<int> id_col(8, -1);   // theta dimension -> column of W_in (identity dimensions only)
    for (int j = 0; j < n.d_id; ++j) id_col[n.idn[j]] = j;
    auto in_col = [&](int it, int rho, bool gate) -> int {   // column of W_in (gate: of W_g) behind an input-tile row
      const int g = rho >> 2, m = rho & 3;
      if (it == 0 && m < 2) { const int dd = 2 * g + m; return (!gate && dd < D) ? id_col[dd] : -1; }
      const int f = it == 0 ? (m - 2) * 4 + g : 8 + (it - 1) * 16 + 4 * m + g;
      if (f >= C) return -1;
      return gate ? f : n.d_id + f;
    };
    auto q_row = [&](int tile, int rho) -> int {   // row of W_out behind a spline-head tile row
      const int g = rho >> 2, sl = 4 * tile + (rho & 3);
      if (g >= n.d_tr) return -1;
      const int fam = sl / KM, kk = sl % KM;
      if (fam > 2 || kk >= (fam < 2 ? K : K - 1)) return -1;
      return g * NP + fam * K + kk;
    };
    // weight functions: rows and columns through the maps above; base = logical offset, ld = its row length
    auto weights = [&](int64_t base, int ld, std::function<int(int, int)> orow, std::function<int(int, int)> icol) -> WFn {
      return [=](int ot, int ro, int it, int ri) -> int64_t {
        const int oo = orow(ot, ro), cc = icol(it, ri);
        return (oo >= 0 && cc >= 0) ? base + (int64_t)oo * ld + cc : -1;
      };
    };
    auto biases = [&](int64_t base, std::function<int(int, int)> orow) -> BFn {
      return [=](int ot, int ro) -> int64_t { const int oo = orow(ot, ro); return oo >= 0 ? base + oo : -1; };
    };
    auto w_gate = [&](int64_t base) { return weights(base, C, hid_unit, [=](int it, int ri) { return in_col(it, ri, true); }); };
    auto w_hid = [&](int64_t base) { return weights(base, H, hid_unit, hid_unit); };
    const WFn w_in = weights(n.Win, n.in_dim, hid_unit, [=](int it, int ri) { return in_col(it, ri, false); });
    const WFn w_out = weights(n.Wout, H, q_row, hid_unit);
    first(c.o_win, c.g_win, ce.fwd(NT, NI, w_in));
    first(c.o_bin, c.g_bin, ce.bias(NT, biases(n.bin, hid_unit)));
    for (int k = 0; k < 2; ++k) {
      first(c.o_wg[k], c.g_wg[k], ce.fwd(NT, NI, w_gate(n.Wg[k])));
      first(c.o_bg[k], c.g_bg[k], ce.bias(NT, biases(n.bg[k], hid_unit)));
      first(c.o_w1[k], c.g_w1[k], ce.fwd(NT, NT, w_hid(n.W1[k])));
      first(c.o_b1[k], c.g_b1[k], ce.bias(NT, biases(n.b1[k], hid_unit)));
      first(c.o_w2[k], c.g_w2[k], ce.fwd(NT, NT, w_hid(n.W2[k])));
      first(c.o_b2[k], c.g_b2[k], ce.bias(NT, biases(n.b2[k], hid_unit)));
    }
    first(c.o_wout, c.g_wout, ce.fwd(OTQ, NT, w_out));
    first(c.o_bout, c.g_bout, ce.bias(OTQ, biases(n.bout, q_row)));
    // LU block: L[8][8], U[8][8], udiag[8], bias[8]; gradient: two 16 x 16 blocks + 16 row sums
    const CoopEmitter::At lu = ce.take(2 * 256 + 16);
    first(c.o_lu, c.g_lu, lu);
    lu_block(n, D, 8, [&](int64_t idx, int64_t g) {
      ce.push(idx);
      if (idx >= 0) ce.owns(idx, lu.g + g);
    });
    while (ce.here() % 16) ce.push(-1);
    // transposed blocks (data gradients)
    first(c.o_woutT, ce.tr(NT, OTQ, w_out));
    for (int k = 0; k < 2; ++k) {
      first(c.o_w2T[k], ce.tr(NT, NT, w_hid(n.W2[k])));
      first(c.o_w1T[k], ce.tr(NT, NT, w_hid(n.W1[k])));
    }
    first(c.o_winT, ce.tr(1, NT, w_in));   // only input tile 0 holds theta dimensions (no context gradient on this path)
    if (t == 0) c.g_stride = (int)((ce.gcur + 63) / 64 * 64);
  }

  // ================================== after the last transform ==================================
  // T == 1: no second transform recorded the strides
  void close_images() {
    E.pad_to(64);
    ET.pad_to(64);
    while (L.srcB.size() % 64) L.srcB.push_back(-1);
    while (L.src16a.size() % 1024) { L.src16a.push_back(-1); L.src16b.push_back(-1); }
    if (T == 1) {
      v.t_stride = (int)E.cur; v.tT_stride = (int)ET.cur; v.tB_stride = (int)L.srcB.size();
      v.t16_stride = (int)L.src16a.size();
    }
  }

  // NSF sampler image: strides, and its staging plan: whole items (input layer | block k: fp32 pieces + split W1 / W2 | head)
  // packed into the LDS budget next to the sampler's control block; no item larger than the budget
  void close_nsf_sampler() {
    SfNsfSamp& sS = L.nsfS;
    while (L.src16a.size() % 64) { L.src16a.push_back(-1); L.src16b.push_back(-1); }
    while (L.src16B.size() % 64) L.src16B.push_back(-1);
    if (T == 1) { sS.t_stride = (int)L.src16a.size(); sS.tB_stride = (int)L.src16B.size(); }
    if (sS.tB_stride & 7) sS.ok = 0;
    if (sS.ok) {
      std::vector<int> cf{0}, cb{0};   // item boundaries: fp32 floats, bf16 elements
      for (int k = 0; k < NB; ++k) { cf.push_back(sS.o_wg[k]); cb.push_back(sS.oB_w1[k]); }
      cf.push_back(sS.o_wout); cb.push_back(sS.tB_stride);
      cf.push_back(sS.t_stride); cb.push_back(sS.tB_stride);
      const Parts p = plan_parts(cf, cb, LDS_BUDGET);
      sS.n_parts = p.n;
      for (int q = 0; q < 5; ++q) { sS.part_off[q] = p.off[q]; sS.partB_off[q] = p.offB[q]; }
      bool okp = p.ok;
      if (okp) {
        for (int q = 0; q < sS.n_parts; ++q) {
          const int pf = sS.part_off[q + 1] - sS.part_off[q], pb = sS.partB_off[q + 1] - sS.partB_off[q];
          sS.part_floats_max = std::max(sS.part_floats_max, pf);
          sS.part_bytes_max = std::max(sS.part_bytes_max, pf * 4 + pb * 2);
          if ((sS.partB_off[q] & 7) || (sS.part_off[q] & 3)) okp = false;   // 16-byte pieces of the direct-to-LDS copies
        }
        for (int k = 0; k < NB; ++k) sS.blk_part[k] = p.item_part[1 + k];
        sS.head_part = p.item_part[1 + NB];
      }
      if (!okp) sS.ok = 0;
    }
    if (!sS.ok) { L.src16a.clear(); L.src16b.clear(); L.src16B.clear(); }
  }

  void close_images16() {
    L.n_packed16 = (int64_t)L.src16a.size();
    if (maf) while (L.src16B.size() % 2048) L.src16B.push_back(-1);
    if (T == 1) v.t16B_stride = (int)(L.src16B.size() / 2);
    L.n_packed16B = (int64_t)L.src16B.size();
    if (!v.m16_ok && !L.nsfS.ok) { L.src16B.clear(); L.n_packed16B = 0; }
    if (v.m16_ok && (size_t)v.t16_stride * sizeof(float) > LDS_BUDGET) v.m16_ok = 0;
    L.n_packedB = (int64_t)L.srcB.size();
  }

  // ---- compact fused image (sf_layout.h, packed16c): where each of its floats sits in a transform of the 16-row image
  // (only for the shapes of the unrolled fused kernels, sf_maf16.hip: D = 3..5 with one hidden tile per degree)
  void compact_image() {
    if (!(maf && v.m16_ok && !v.m16_span && v.o16_wp >= 0 && v.o16_wh >= 0 && NB <= 2 && D >= 3 && D <= 5 && v.nT16 == D - 1)) return;
    const int NT = v.nT16;
    auto run = [&](int from, int n) { for (int i = 0; i < n; ++i) L.src16c.push_back(from + i); };
    auto align = [&](size_t q) { while (L.src16c.size() % q) L.src16c.push_back(-1); };
    auto here = [&]() { return (int)L.src16c.size(); };
    v.o16c_bk1 = here();
    if (NB == 2) run(v.o16_bk[1], NT * 16);
    v.o16c_hvb = here();
    run(v.o16_hvb, 2 * D);
    align(4);
    v.o16c_bh = here();
    run(v.o16_bh, 16);
    v.o16c_wh = here();
    run(v.o16_wh, NT * 256);
    v.o16c_wp = here();
    const int KN = std::min(NT, D - 1);   // (k_maf_fuse16: the dimension of degree D feeds nothing)
    run(v.o16_wp, (KN * NT - KN * (KN - 1) / 2) * 16);
    v.o16c_blk = here();
    if (NB == 2)
      for (int ot = 0; ot < NT; ++ot)
        for (int it = 0; it <= ot; ++it) run(v.o16_wk[1] + (ot * NT + it) * 256, 256);
    align(256);
    v.t16c_stride = here();
    // ---- head rows of the per-lane form (sf_pass16g), behind the compact image of each transform: one entry of 32 floats
    // [g4][r][a|m] per (hidden tile ot, degree k >= ot + 2), tiles in order and each with its degrees in order (sf_hr16_entry), from
    // the o16_hv rows of the slot that holds degree k IN THAT TRANSFORM -- hence one table per transform
    const int NE = D * (D - 1) / 2;
    v.t16h_stride = (NE * 32 + 255) / 256 * 256;
    L.src16h.assign((size_t)T * v.t16h_stride, -1);
    for (int tt = 0; tt < T; ++tt) {
      int32_t* th = L.src16h.data() + (size_t)tt * v.t16h_stride;
      int e = 0;
      for (int ot = 0; ot < NT; ++ot)
        for (int k = ot + 2; k <= D; ++k, ++e)
          for (int g4 = 0; g4 < 4; ++g4)
            for (int i = 0; i < 8; ++i) th[e * 32 + g4 * 8 + i] = v.o16_hv + sigma[tt][k - 1] * 128 + g4 * 32 + ot * 8 + i;
    }
  }

  // ---- LDS staging plan of the main image: MAF one item; NSF the input layer | block k from its gate weights on | the spline
  // head + the small LU block (LU is used from LDS only when n_parts == 1).  false: hidden_bf16 does not fit.
  bool staging_plan() {
    std::vector<int> cuts{0};  // block boundaries (float offsets) in execution order, first = 0, last = end
    if (!maf) {
      for (int k = 0; k < NB; ++k) cuts.push_back(v.o_wg[k]);
      cuts.push_back(v.o_wout);
    }
    cuts.push_back(v.t_stride);
    const Parts p = plan_parts(cuts, std::vector<int>(cuts.size(), 0), LDS_BUDGET);
    for (int q = 0; q < 5; ++q) v.part_off[q] = p.off[q];
    v.n_parts = p.ok ? p.n : 0;
    if (p.ok) {
      for (int q = 0; q < v.n_parts; ++q) v.part_max = std::max(v.part_max, v.part_off[q + 1] - v.part_off[q]);
      if (!maf) {
        for (int k = 0; k < NB; ++k) v.blk_part[k] = p.item_part[1 + k];
        v.head_part = p.item_part[1 + NB];
      }
    }
    for (int q = 0; q < 5; ++q) v.partB_off[q] = q == 0 ? 0 : v.tB_stride;   // (single-part bf16 images: everything with part 0)
    v.part_bytes_max = v.part_max * 4 + (v.hidden_bf16 ? v.tB_stride * 2 : 0);
    // hidden_bf16: the fp32 image + the bf16 image of one transform in one part
    return !v.hidden_bf16 || (v.n_parts == 1 && (size_t)(v.t_stride + (v.tB_stride + 1) / 2) * 4 <= LDS_BUDGET);
  }

  void close_coop() {
    if (!L.trc.ok && !L.nsc.ok) return;
    while (L.srcC1.size() % 256) { L.srcC1.push_back(-1); L.srcC2.push_back(-1); }
    if (T == 1) { L.trc.t_stride = (int)L.srcC1.size(); L.nsc.t_stride = (int)L.srcC1.size(); }
    L.n_imgC = (int64_t)L.srcC1.size();
    L.n_gradC = (int64_t)T * (L.trc.ok ? L.trc.g_stride : L.nsc.g_stride);
    L.gdstC.resize((size_t)P, -1);
    // position -> parameter(s) for the gather.  A position feeds at most two parameters; a layout that maps more (none the
    // builder emits) has no cooperative image at all and trains with the 32-row kernels
    L.gsrcC.assign((size_t)L.n_gradC * 2, -1);
    L.gzeroC.clear();
    bool ok = true;
    for (int64_t i = 0; i < P && ok; ++i) {
      const int32_t g = L.gdstC[(size_t)i];
      if (g < 0) { L.gzeroC.push_back((int32_t)i); continue; }
      int32_t* slot = g < L.n_gradC ? &L.gsrcC[(size_t)g * 2] : nullptr;
      if (slot && slot[0] < 0) slot[0] = (int32_t)i;
      else if (slot && slot[1] < 0) slot[1] = (int32_t)i;
      else ok = false;
    }
    if (!ok) { L.trc.ok = 0; L.nsc.ok = 0; L.gsrcC.clear(); L.gzeroC.clear(); }
  }

  // gradient image of the 32-row path: the first image copy of a parameter owns its gradient
  void gradient_map() {
    L.n_packed = E.cur;
    L.n_packedT = ET.cur;
    L.n_params = P;
    L.gdst.assign((size_t)P, -1);
    for (int64_t i = 0; i < E.cur; ++i) {
      if (L.src1[i] >= 0 && L.gdst[L.src1[i]] < 0) L.gdst[L.src1[i]] = gidx[i];
      if (L.src2[i] >= 0 && L.gdst[L.src2[i]] < 0) L.gdst[L.src2[i]] = gidx[i];
    }
  }
};

}  // namespace

bool sf_build_layout(const sf_flow_desc& d, SfLayout& L) {
  if (const char* e = desc_error(d)) {
    L.error = e;
    return false;
  }
  return LayoutBuilder(d, L).run();
}

// =============================================================================================
// embedding MLP
// =============================================================================================
bool sf_build_mlp_layout(const sf_mlp_desc& d, SfMlpLayout& L) {
  auto fail = [&](const std::string& m) { L.error = m; return false; };
  if (d.n_in < 1 || d.n_in > 512) return fail("n_in must be in 1..512");
  if (d.n_layers < 1 || d.n_layers > SF_MLP_LMAX) return fail("n_layers must be in 1..4");
  if (d.act < 0 || d.act > 2) return fail("unknown activation");
  int wmax = 0;
  for (int l = 0; l < d.n_layers; ++l) {
    if (d.widths[l] < 1 || d.widths[l] > 128) return fail("layer widths must be in 1..128");
    wmax = std::max(wmax, d.widths[l]);
  }
  SfMlpDev& v = L.dev;
  std::memset(&v, 0, sizeof(v));
  v.n_in = d.n_in; v.L = d.n_layers; v.act = d.act; v.n_out = d.widths[d.n_layers - 1];
  v.HT = ceil_div(wmax, 32);
  L.cst.assign(2 * ((d.n_in + 3) / 4) * 4, 1.f);
  for (int i = 0; i < d.n_in; ++i) {
    L.cst[i] = d.x_mean ? d.x_mean[i] : 0.f;
    L.cst[((d.n_in + 3) / 4) * 4 + i] = d.x_std ? d.x_std[i] : 1.f;
  }
  std::vector<int32_t> gidx;
  Emitter E{L.src1, L.src2, &gidx};
  Emitter ET{L.srcT1, L.srcT2, nullptr};
  int64_t P = 0;
  int in_w = d.n_in;
  for (int l = 0; l < d.n_layers; ++l) {
    const int out_w = d.widths[l];
    v.width[l] = out_w;
    v.nG[l] = ceil_div(in_w, 8);
    v.nGo[l] = ceil_div(out_w, 8);
    const int64_t lW = P, lb = lW + (int64_t)out_w * in_w;
    P = lb + out_w;
    E.pad_to(64);
    v.o_w[l] = (int)E.linear(v.HT, v.nG[l], iota_rows(out_w, v.HT * 32), iota_rows(in_w, v.nG[l] * 8), lW, in_w, 1, nullptr);
    v.o_b[l] = (int)E.bias(v.HT, iota_rows(out_w, v.HT * 32), lb, -1);
    if (l > 0) {  // delta_in = W^T delta_out : rows = previous layer's units, K = this layer's outputs
      ET.pad_to(64);
      v.oT_w[l] = (int)ET.linear(v.HT, v.nGo[l], iota_rows(in_w, v.HT * 32), iota_rows(out_w, v.nGo[l] * 8), lW, 1,
                                 in_w, nullptr);
    }
    in_w = out_w;
  }
  E.pad_to(64);
  ET.pad_to(64);
  L.n_packed = E.cur;
  L.n_packedT = ET.cur;
  L.n_params = P;
  L.gdst.assign((size_t)P, -1);
  for (int64_t i = 0; i < E.cur; ++i)
    if (L.src1[i] >= 0) L.gdst[L.src1[i]] = gidx[i];
  return true;
}
