// sf_internal.h -- launcher prototypes shared by the kernel translation units and sf_api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sf_buf.h"
#include "sf_layout.h"
#include "sf_queue.h"

struct SfSampleArgsHost {
  const float* x = nullptr;
  const float* z_in = nullptr;
  long S = 1;
  const uint32_t* slots = nullptr;
  long slot_base = 0;
  long n_items = 0;
  uint32_t attempt = 0, k0 = 0, k1 = 0;
  // added to the slot id in the Philox counter only: row_offset * S, so that a block of rows of a larger catalogue
  // (a chunk, a rank's shard) draws exactly what those rows draw in a single call over the whole catalogue
  unsigned long long rng_slot_offset = 0;
  int attempts_per_slot = 1;  // A: consecutive attempts evaluated per listed slot (power of two <= 32)
  int log2_attempts = 0;      // log2(A) (set by sf_launch_inverse)
  const float* lo = nullptr;
  const float* hi = nullptr;
  float* out = nullptr;
  int out_f64 = 0;            // != 0: `out` is a double array (sf_flow_set_sample_output_f64): accepted draws are widened in the store
  float* logdet_out = nullptr;
  uint32_t* rejected = nullptr;
  uint32_t* n_rejected = nullptr;
  int32_t* n_drawn = nullptr;
  int32_t* count = nullptr;
  // find mode (plain kernels): listed slot i = item >> log2_attempts (any power of two of attempts per slot); an accepted
  // attempt only lowers best[i] (atomic min), nothing else is written.  att_list (sampling mode, attempts_per_slot 1):
  // listed slot i tries attempt att_list[i] instead of `attempt` (0xffffffff = none: goes straight to the rejected list)
  uint32_t* best = nullptr;
  const uint32_t* att_list = nullptr;
  // persistent mode (q != nullptr): one launch works the dense list AND its retries to the end (sf_queue.h)
  struct SfQueue* q = nullptr;
  unsigned long long* ring = nullptr;  // retry ring, ring_mask + 1 entries
  uint32_t ring_mask = 0;
  uint32_t attempt_limit = 0xffffffffu;  // attempts [attempt, attempt_limit) are tried by this launch; then -> rejected[]
  uint32_t n_total = 0;                // slots of the dense list (== n_items)
  uint32_t out_slots = 0;              // M * S: every slot id must be below this
  // != 0 (whole-catalogue launches: slots == nullptr, slot_base == 0, n_total == M * S): the dense list walks ACROSS the
  // galaxies inside blocks of dense_G consecutive galaxies -- item i lies in block b = i / (dense_G * S); with Gb =
  // min(dense_G, M - b * dense_G) galaxies in that block and j = i - b * dense_G * S it is slot
  // (b * dense_G + j % Gb) * S + j / Gb.  In plain slot order the ~8 workgroups that draw the ranges of a low-acceptance
  // galaxy grind through its retries alone while the rest of the chip runs dry (their own retries come first and the dense
  // phase does not share work); interleaved, every workgroup carries the same mix, and a block keeps the context rows
  // in flight few enough to stay cached.  The draws do not depend on the order (streams are keyed by slot and attempt).
  uint32_t dense_G = 0;
  // ... in RUNS of dense_run consecutive draws of one galaxy (dense_run divides S; 1 = draw by draw): with a run = one tile
  // of draws (16 / 32) the lanes of a tile share their galaxy's context-table rows and write one contiguous piece of the
  // output, and a galaxy's S slots still spread over S / dense_run ranges.  Within a block of Gb galaxies item j is draw
  // (j / run / Gb) * run + j % run of galaxy (j / run) % Gb.
  uint32_t dense_run = 1;
  // != 0 (an explicit slot list, e.g. an ensemble member's share, sorted by slot): item i of the dense list is list entry
  // walk(i), walk = i -> i * list_mul mod 2^list_log2, repeated until the result is < n_total (cycle walking: a
  // permutation of [0, n_total)) -- consecutive items lie ~n_total / 128 entries apart, for the same reason as dense_G
  uint32_t list_mul = 0, list_log2 = 0;
  int32_t* gal_acc = nullptr;          // optional [M]: += 1 per accepted slot of the galaxy (progress test between stages)
#ifdef SF_Q_STATS
  // developer build: [workgroup][256][4] = {start of the iteration (10 ns since the first workgroup's start is taken on
  // the host), entries, log2 attempts per entry, end of its epilogue} of every iteration of every workgroup
  uint32_t* qtrace = nullptr;
#endif
};
#ifdef __HIPCC__
// one value of an accepted draw: fp32 into a float array or -- out_f64 -- widened into a double array (wave-uniform choice)
__device__ __forceinline__ void sf_out_store(const SfSampleArgsHost& a, size_t idx, float v) {
  if (a.out_f64) reinterpret_cast<double*>(a.out)[idx] = (double)v;
  else a.out[idx] = v;
}
#endif

// What a density-direction kernel writes per row, each unless NULL: lp = log q(theta | x) (sf_flow_log_prob), z[B, D] = the
// latent T(theta; x) in the column order sf_flow_inverse_from_noise reads, lad = log |det dz / dtheta| with the standardisation
// term (sf_flow_to_noise).  z_vec: the rows of z are 16-byte aligned (D % 4 == 0 and the base is) and leave as 16-byte pieces,
// decided once on the host (sf_lp_out).
struct SfLpOut {
  float* lp = nullptr;
  float* z = nullptr;
  float* lad = nullptr;
  int z_vec = 0;
};
inline SfLpOut sf_lp_out(float* lp, float* z, float* lad, int D) {
  SfLpOut o;
  o.lp = lp; o.z = z; o.lad = lad;
  o.z_vec = (z && (D & 3) == 0 && (reinterpret_cast<uintptr_t>(z) & 15) == 0) ? 1 : 0;
  return o;
}

hipError_t sf_launch_logprob(const SfDev& m, const float* theta, const float* x, long B, SfLpOut out,
                             hipStream_t st);
hipError_t sf_launch_inverse(const SfDev& m, const SfSampleArgsHost& a, hipStream_t st);
bool sf_maf16_enabled(const SfDev& m, const SfSampleArgsHost& a);
hipError_t sf_launch_maf_inv16(const SfDev& m, const SfSampleArgsHost& a, hipStream_t st);
hipError_t sf_launch_maf_inv16b_hook(const SfDev& m, const float* z, const float* x, long n, float* out, hipStream_t st);
void sf_sampler_fp32_set(int on);
int sf_sampler_fp32_get();        // 1 fp32, 0 split bf16 x3, -1 unset: per flow kind
int sf_sampler_fp32_for(int kind);  // the mode a flow of this kind samples in (unset: MAF fp32, NSF split)
// per-galaxy context table: rows/variants for this flow (0 = the flow has no table path), builder
void sf_ctab_shape(const SfDev& m, int& R, int& NV);
hipError_t sf_launch_ctab(const SfDev& m, const float* x, long M, float* tab, hipStream_t st);
hipError_t sf_launch_maf_ctab16(const SfDev& m, const float* x, long M, float* tab, hipStream_t st);
hipError_t sf_launch_maf_fuse16(const SfDev& m, hipStream_t st);   // W' = (W1 o M)(W0 o M0) into o16_wp of every transform
// the compact fused image of every transform from the 16-row image (after sf_launch_maf_fuse16: it carries W'); tab: per transform SfLayout::src16c, then that
// transform's part of src16h
hipError_t sf_launch_maf_compact16(const SfDev& m, const int32_t* tab, float* out, hipStream_t st);
// the compact image's offsets against the compile-time ones of the unrolled fused kernels: 1 equal, 0 not, -1 no such kernel for the shape
int sf_maf16_compact_fix(const SfDev& m);
// Which 16-row MAF kernels (sf_maf16.hip) a view of a flow runs on, in the process's sampler arithmetic: the one place that decides.
struct SfMaf16Plan {
  bool ok16 = false;       // the flow has the 16-row path at all (fp32 image; sf_maf16_enabled adds the launch's own condition)
  bool sampler16 = false;  // ... and its persistent sampler in this arithmetic; false: the sampler IS the 32-row fp32 path
  bool fp32 = false;       // hidden blocks in fp32 (sf_sampler_fp32_for(SF_MAF)), else split bf16 x3
  bool span = false;       // contiguous placement: degree groups straddle tiles
  bool head_mfma = false;  // head rows on the matrix pipe (aligned placement with the head tile in the image: D <= 8)
  int dd = 0;              // D (3..5) when the unrolled kernels apply (this view has the context table, degree p alone in tile p - 2,
                           // the packer's offsets are the hard-wired ones), else 0: the kernels that dispatch per pass
  bool fused = false;      // ... with the fused first layer (fp32, the table carries the c0' rows, the compact image is fresh and
                           // the packer's offsets in it are the hard-wired ones)
};
SfMaf16Plan sf_maf16_plan(const SfDev& m);
hipError_t sf_launch_maf_find16_zin(const SfDev& m, const SfSampleArgsHost& a, hipStream_t st);
hipError_t sf_launch_pack(const float* flat, const int32_t* s1, const int32_t* s2, float* packed, long n,
                          hipStream_t st);
hipError_t sf_launch_pack_bf16(const float* flat, const int32_t* src, unsigned short* out, long n, hipStream_t st);
hipError_t sf_launch_pack_bf16_split(const float* flat, const int32_t* src, unsigned short* out, long n, hipStream_t st);
hipError_t sf_launch_fill_nan_rows(float* out, const uint32_t* slots, long n, int D, hipStream_t st, int out_f64 = 0);
hipError_t sf_launch_fill_i32(int32_t* p, long n, int32_t v, hipStream_t st);
// exclusive scan of n int32 counts by one workgroup (the sum stays below 2^31): offs[0..n), and the sum to *total unless null
hipError_t sf_launch_exclusive_scan_i32(const int32_t* cnt, int n, int32_t* offs, int32_t* total, hipStream_t st);
hipError_t sf_launch_account_window(const uint32_t* list, const uint32_t* best, long n, long S, uint32_t a_lo, uint32_t A,
                                    int32_t* n_drawn, int32_t* gal_acc, hipStream_t st);
// survivors of galaxies with gal_acc == 0 become NaN rows; the others are compacted in place; *n_surv updated
hipError_t sf_launch_filter_survivors(uint32_t* list, unsigned int* n_surv, long S, const int32_t* gal_acc, float* out,
                                      int D, hipStream_t st, int out_f64 = 0);

#include <string>
#define SF_MAX_DEVICES 16   // devices of one process that per-device host state (attribute caches, tool scratch) has a slot for
// per-device "attribute already set" cache for hipFuncSetAttribute(MaxDynamicSharedMemorySize): function attributes are
// per device, so a process that launches on a second device must set them there too
struct SfAttrCache {
  bool done[SF_MAX_DEVICES] = {false};
  bool need(int& dev) {
    dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= SF_MAX_DEVICES) return true;
    return !done[dev];
  }
  void set(int dev) { if (dev >= 0 && dev < SF_MAX_DEVICES) done[dev] = true; }
};
// resident workgroups of a persistent kernel, cached per (device, dynamic LDS bytes): the occupancy of one template instance
// depends on the flow's LDS footprint and the grid on the device's CU count -- a process that samples flows of different
// sizes, or on a second GPU, must not reuse the first answer
struct SfResidentCache {
  int dev[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
  size_t sh[8] = {0};
  int val[8] = {0};
  int n = 0;
  bool get(int d, size_t s, int& v) const {
    for (int i = 0; i < 8; ++i)
      if (dev[i] == d && sh[i] == s) { v = val[i]; return true; }
    return false;
  }
  void put(int d, size_t s, int v) { dev[n & 7] = d; sh[n & 7] = s; val[n & 7] = v; ++n; }
};
void sf_set_error(const std::string& msg);          // thread-local message behind sf_last_error()
int sf_fail(int code, const std::string& msg);      // sf_set_error(msg), then `code` for the caller to return
// a HIP call that must succeed: on failure the message "<call>: <hip error>" becomes the thread's last error and the enclosing
// function returns SF_ERR_HIP.  (An operation of an owner, sf_buf.h -- x.alloc(n), x.grow(n), x.upload(v), x.create() -- also names the runtime function that failed.)
inline std::string sf_hip_message(const char* call, hipError_t e) {
  std::string s = std::string(call) + ": ";
  for (const char* op : {".alloc(", ".grow(", ".upload(", ".create("})
    if (s.find(op) != std::string::npos) { s += std::string(sf_buf_last_call()) + ": "; break; }
  return s + hipGetErrorString(e);
}
#define SF_TRY_SET(call)                                                                                   \
  do {                                                                                                     \
    hipError_t e_ = (call);                                                                                \
    if (e_ != hipSuccess) return sf_fail(SF_ERR_HIP, sf_hip_message(#call, e_));                          \
  } while (0)
struct sf_comm;
int sf_comm_all_reduce_impl(sf_comm* c, float* buf, long n, hipStream_t st);  // sf_comm.hip: ncclAllReduce(SUM, fp32) in place

// ---- the handle (shared by sf_api.hip, sf_train.hip and sf_gradtheta.hip) ----------------------
// Every d_* / h_* / ev_* member owns what it points to (sf_buf.h): sf_flow_destroy is `delete`.  Buffers that are built together,
// all or nothing, form a struct that the handle inherits (so that their names read as before): the builder fills a local one and
// moves it in, and a group that has to grow is first assigned an empty one (free before malloc).
#define SF_LOSS_PARTS 64
struct SfNsf1;
struct SfFlowDev {   // ensure_device (sf_api.hip)
  SfBuf<float> d_packed;        // forward operand image
  SfBuf<float> d_cst;
  SfBuf<int32_t> d_s1, d_s2;
  SfBuf<float> d_packed16;      // 16-row image of the incremental MAF inverse (sf_maf16.hip)
  SfBuf<int32_t> d_s16a, d_s16b;
  SfBuf<float> d_packed16c;     // compact fused image (sf_layout.h: packed16c), rebuilt with W' (wp_stale)
  SfBuf<int32_t> d_s16c;        // its gather table and the head rows' behind it, [T][t16c_stride + t16h_stride]
  SfBuf<unsigned short> d_packed16B;  // split-bf16 hidden blocks of the 16-row sampler (sf_layout.h)
  SfBuf<int32_t> d_s16B;
  SfBuf<unsigned short> d_packedB;    // bf16 hidden operand image (hidden_bf16)
  SfBuf<int32_t> d_bsrc;
  SfBuf<float> d_flat;          // staging for host-sourced parameters
  SfEvent ev_dense[2];          // brackets round 0 of the last sf_flow_sample call
};
struct SfFlowTrain {   // the `train_ready` group (sf_train.hip)
  SfBuf<float> d_packedT;       // transposed operand image (training, lazily built)
  SfBuf<int32_t> d_t1, d_t2;
  SfBuf<float> d_gpacked;       // gradient image replicas (accumulation target)
  SfBuf<int32_t> d_gdst;        // logical parameter -> gradient image index
};
struct SfFlowTrainC {  // the `trainc_ready` group: cooperative 16-row training path (sf_trainc.hip), operand image and gather tables
  SfBuf<float> d_imgC;
  SfBuf<int32_t> d_sC1, d_sC2;
  SfBuf<int32_t> d_gsrcC;       // SfLayout::gsrcC: [n_gradC][2] parameters fed by a position of the gradient partial (-1: none)
  SfBuf<int32_t> d_gzeroC;      // SfLayout::gzeroC: parameters without a position (their gradient is 0)
  long n_gzeroC = 0;
};
// transposed INFERENCE image of sf_flow_log_prob_grad (sf_gradtheta.hip): built from d_flat on the first gradient call after
// sf_flow_set_params, valid until the next one; buffers of its own, training's d_packedT is rebuilt per call from the caller's vector
struct SfFlowGt {
  SfBuf<float> d_gtT;
  SfBuf<int32_t> d_gt1, d_gt2;
};
struct SfFlowRej { SfBuf<uint32_t> d_rej[2]; };   // rejected-slot lists of the persistent sampler, one capacity
struct sf_flow : SfFlowDev, SfFlowTrain, SfFlowTrainC, SfFlowGt, SfFlowRej {
  SfLayout L;
  struct SfNsfAr* nsfar = nullptr;   // != null: the autoregressive NSF (sf_nsfar.hip); L carries the shape and n_params only
  SfNsf1* nsf1 = nullptr;       // != null: the one-parameter NSF (sf_nsf1.hip); L then only carries the shape and n_params
  ~sf_flow();                   // sf_api.hip: the two sub-handles
  bool dev_ready = false;
  bool params_set = false;
  bool train_ready = false;     // every lazily built training buffer exists (sf_train.hip)
  bool flat_valid = false;      // d_flat holds the vector last given to sf_flow_set_params
  bool gt_image_valid = false;
  long gt_simds = 0;            // SIMDs of the handle's device (4 per CU), asked once: the width a stash-bounded launch keeps
  bool packed16_stale = false;          // loss_grad refreshed only the forward image
  SfBuf<float> d_gpartC;        // cooperative training: gradient partials
  SfBuf<long long> d_gfixC;     // SF_FIX_REPLICAS int64 gradient images (fixed-point accumulation, sf_fixacc.h)
  bool trainc_ready = false;
  SfBuf<float> d_ustash;        // cooperative NSF training (sf_nsfc.hip): u / u' of every transform, [rows][T][16]
  SfBuf<float> d_act;           // activation stash (training)
  SfBuf<SfQueue> d_queue;       // work-queue words of the persistent sampler (sf_queue.h)
  SfPinned<SfQueue> h_queue;    // pinned host mirror, read once per stage
  SfBuf<unsigned long long> d_ring;  // retry ring (a power of two of entries)
  bool ring_dirty = false;       // a persistent launch did not end cleanly: clear the ring before the next one
  SfBuf<int32_t> d_galacc;       // per-galaxy accepted-slot counter of a stage (progress rule)
  SfBuf<uint32_t> d_best;        // deep-tail windows: lowest accepted attempt per survivor (find launch -> resolve launch)
  // per-block shares of |grad|^2 from the gather of the last loss_grad (epoch loop only: want_sq); n_sqpart = 0: none
  SfBuf<float> d_sqpart;
  int n_sqpart = 0;
  bool want_sq = false;
  bool prep_lite = false;     // epoch call, not its last step: only the cooperative training image is re-tiled per step
  bool packed_stale = false;  // the density / sampler images lag behind the training image (cleared by the next full re-tiling)
  // loss sums of an epoch call spread over SF_LOSS_PARTS device scalars (non-null only inside sf_flow_train_epoch), folded into
  // the caller's scalar at its end
  double* d_losspart = nullptr;      // (a view of d_losspart_mem, not an owner)
  SfBuf<double> d_losspart_mem;
  bool losspart_used = false;
  bool wp_stale = true;              // the fused first-layer blocks (o16_wp) and the compact image (d_packed16c) lag behind packed16:
                                     // recomputed before the next context table
  bool sample_out_f64 = false;       // sf_flow_set_sample_output_f64: `out` of sf_flow_sample / _slots is a double array
  long long sample_row_offset = 0;   // sf_flow_set_sample_row_offset: first row of the next sampling calls in its catalogue
  double sample_time_limit_s = 0.0;  // > 0: sf_flow_sample* stop opening new attempt windows after this much wall time
  bool profiling = false;         // sf_flow_set_profiling: bracket the training flow kernel with HIP events
  SfEvent ev_train[2];
  bool ev_train_valid = false;
  float last_stats[4] = {0.f, 0.f, 0.f, 0.f};   // dense-round ms, rounds, rejected after round 0, items evaluated
  SfBuf<float> d_ctab;           // per-galaxy context table (sf_flow_prepare_context)
  const float* ctab_x = nullptr; // context rows the table was built from (NULL = no valid table)
  int64_t ctab_M = 0;
  SfDev dev() const {
    SfDev v = L.dev;
    v.packed = d_packed;
    v.packedT = d_packedT;
    v.cst = d_cst;
    v.packedB = d_packedB;
    v.packed16 = packed16_stale ? nullptr : d_packed16.get();
    v.packed16B = reinterpret_cast<const uint32_t*>(d_packed16B.get());
    v.packed16c = (packed16_stale || wp_stale) ? nullptr : d_packed16c.get();
    v.ctab = nullptr;  // set per launch by the sampler entry points
    return v;
  }
};

// device fp32 -> host float64 hand-over (sf_hostio.hip)
int sf_hostio_copy_f64(const float* dev_src, double* host_dst, int64_t n, hipStream_t stream);
