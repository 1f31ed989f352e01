/*
 * synference_hip.h -- C ABI of the MI355X (gfx950) amortised-posterior flow engine.
 *
 * Drop-in boundary for ONE path of synthesizer-project/synference: the conditional
 * normalizing-flow density estimator (MAF / NSF) that the reference reaches through
 *     ili.utils.load_nde_sbi(...)            ref: src/synference/sbi_runner.py:5123-5146
 *     estimator_builder(batch_x=, batch_theta=)   ref: src/synference/custom_runner.py:320-326
 * and evaluates through
 *     posterior.sample((S,), x=)             ref: src/synference/sbi_runner.py:6438-6442
 *     posterior.log_prob(x=, theta=)         ref: src/synference/sbi_runner.py:7193-7196
 *     loss.backward(); clip; optimizer.step()  ref: src/synference/custom_runner.py:585-618
 *
 * The reference is pure Python (no FFI of its own), so these entry points are what a
 * ctypes binding for that path would bind; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - plain pointers and sizes only; every data pointer is a DEVICE pointer to
 *     contiguous row-major float32 unless the comment says "host".
 *   - the caller owns every buffer it passes; the library owns the handle, its packed
 *     weight image and its scratch.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are
 *     asynchronous on it unless stated.
 *   - return 0 on success, a negative sf_status otherwise; sf_last_error() returns the
 *     thread-local message.
 *   - one handle per (process, device); a handle is not thread-safe.
 *
 * Logical parameter layout (the flat vector of sf_flow_set_params / sf_flow_loss_grad),
 * per transform t = 0..T-1, torch nn.Linear convention W[out][in], row-major:
 *   MAF: W0[H,D] b0[H] Wc[H,C] bc[H] {Wk[H,H] bk[H]} x NB  Wf[2D,H] bf[2D]
 *   NSF: Win[H,d_id+C] bin[H] {Wg[H,C] bg[H] W1[H,H] b1[H] W2[H,H] b2[H]} x NB
 *        Wout[d_tr*(3K-1),H] bout[d_tr*(3K-1)]
 *        and, when D > 1: lower[D(D-1)/2] upper[D(D-1)/2] udiag[D] lubias[D]
 *        (tril / triu index order, row-major, as numpy tril_indices(D,-1) / triu_indices(D,1))
 *   NSF_AR: W0[H,D+C] b0[H] W1[H,H] b1[H] W2[D*(3K-1),H] b2[D*(3K-1)]   (NB = 2 hidden layers; row d*(3K-1)+j of the
 *        head: j in [0,K) widths, [K,2K) heights, [2K,3K-1) derivatives of dimension d; tail_bound = zuko's `bound` [5])
 * MADE masks are implied by (D, H) and applied inside the library (masked entries of
 * the flat vector are ignored on input and receive zero gradient).
 */
#ifndef SYNFERENCE_HIP_H
#define SYNFERENCE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sf_flow sf_flow;
typedef struct sf_opt sf_opt;

enum sf_status {
  SF_OK = 0,
  SF_ERR_INVALID = -1,     /* bad argument / unsupported shape */
  SF_ERR_HIP = -2,         /* a HIP runtime call failed */
  SF_ERR_NO_DEVICE = -3,   /* no gfx950 device visible */
  SF_ERR_STATE = -4        /* e.g. parameters not set */
};

/* SF_NSF_AR: the autoregressive NSF of the reference's second backend (backend="lampe" -> zuko.flows.NSF;
 * ref: src/synference/sbi_runner.py:5123-5125): masked hyper-network + zuko's monotonic rational-quadratic spline */
/* SF_MAF_AR: the MAF of the same backend (backend="lampe", model "maf" -> zuko.flows.MAF, sbi_runner.py:5123-5125): the same masked
 * hyper-network with two outputs per dimension and zuko's MonotonicAffineTransform as the univariate map
 * (y = x exp(s / (1 + |s / log slope|)) + shift); K, tail_bound and the spline fields are ignored. */
enum sf_kind { SF_MAF = 0, SF_NSF = 1, SF_NSF_AR = 2, SF_MAF_AR = 3 };

/* Static description of one flow.  Pointer members are HOST arrays read during
 * sf_flow_create only.  Defaults of the upstream stack (sbi/nflows) in brackets. */
typedef struct sf_flow_desc {
  int32_t kind;            /* sf_kind */
  int32_t D;               /* theta dimension, 1..16 */
  int32_t C;               /* context width seen by the transforms, 1..512 */
  int32_t H;               /* hidden_features [50], 1..128 */
  int32_t T;               /* num_transforms [5] */
  int32_t K;               /* num_bins (NSF) [10], 2..16 */
  int32_t NB;              /* num_blocks [2], 1..4 */
  int32_t scale_fn;        /* MAF scale: 0 = softplus(a)+eps [nflows>=0.14], 1 = sigmoid(a+2)+eps */
  int32_t hidden_bf16;     /* 0 = fp32 everywhere [default]; 1 = the hidden H x H layers of the INFERENCE kernels
                              (log_prob / inverse / sampler) use bf16 MFMA operands with fp32 accumulation
                              (BASELINE configs[4]); everything else, and all training, stays fp32 */
  float tail_bound;        /* [3.0] */
  float min_bin_width;     /* [1e-3] */
  float min_bin_height;    /* [1e-3] */
  float min_derivative;    /* [1e-3] */
  float maf_eps;           /* [1e-3] */
  float lu_eps;            /* [1e-3] */
  const float* theta_mean; /* host [D]  z-score buffers (sbi standardizing_transform) */
  const float* theta_std;  /* host [D] */
  const float* x_mean;     /* host [C]  (sbi standardizing_net) */
  const float* x_std;      /* host [C] */
  const int32_t* perms;    /* host [T*D] MAF RandomPermutation buffers, NULL = identity */
  float ar_slope;          /* SF_NSF_AR: slope of zuko's MonotonicRQSTransform [1e-3]; ignored by the other kinds */
} sf_flow_desc;

/* ---- lifetime ---------------------------------------------------------------------- */
/* Builds the layer tables and allocates the packed weight image on the current device.
 * Replaces: the nn.Module returned by build_fn (custom_runner.py:326). */
int sf_flow_create(const sf_flow_desc* desc, sf_flow** out);
void sf_flow_destroy(sf_flow* f);
int64_t sf_flow_num_params(const sf_flow* f);
/* floats in the MFMA-tiled weight image (for tests / diagnostics) */
int64_t sf_flow_packed_size(const sf_flow* f);

/* ---- parameters -------------------------------------------------------------------- */
/* flat: n = sf_flow_num_params floats in the logical layout; is_device selects host or
 * device source.  Re-tiles them into the MFMA operand image (a device gather kernel).
 * Replaces: estimator.load_state_dict (custom_runner.py:563, 709). */
int sf_flow_set_params(sf_flow* f, const float* flat, int64_t n, int is_device, void* stream);

/* Copies the logical vector last given to sf_flow_set_params back out (host or device destination).
 * SF_ERR_STATE after sf_flow_loss_grad*: during training the caller's vector is the master copy.
 * Replaces: estimator.state_dict() (custom_runner.py:658). */
int sf_flow_get_params(sf_flow* f, float* flat, int64_t n, int is_device, void* stream);

/* Host-only helpers (no GPU needed; used by the CPU test-suite):
 * src1/src2[i] = logical index feeding packed float i (or -1); packed = sum of both. */
int sf_flow_pack_table(const sf_flow* f, int32_t* src1, int32_t* src2, int64_t n_packed);
/* the same for the 16-row image of the incremental MAF sampler (size 0 when the flow has none) */
int64_t sf_flow_packed16_size(const sf_flow* f);
int sf_flow_pack_table16(const sf_flow* f, int32_t* src1, int32_t* src2, int64_t n_packed16);
/* split-bf16 image of the hidden blocks of the persistent 16-row sampler: src[i] = logical index | (part << 30) for
 * bf16 element i (part 0: hi = bf16(w), part 1: lo = bf16(w - hi)), -1 = zero; size 0 when the flow has none */
int64_t sf_flow_packed16b_size(const sf_flow* f);
int sf_flow_pack_table16b(const sf_flow* f, int32_t* src, int64_t n);
/* compact image of the fused fp32 16-row sampler (csrc/sf_layout.h, packed16c): floats per transform (0 when the flow has none)
 * and, for ONE transform, src[i] = offset of float i inside that transform of the 16-row image, -1 = padding */
int64_t sf_flow_packed16c_size(const sf_flow* f);
int sf_flow_pack_table16c(const sf_flow* f, int32_t* src, int64_t n);
/* head rows behind the compact image (csrc/sf_layout.h, t16h_stride): T x t16h_stride entries (0 when the flow has none),
 * src[t * t16h_stride + i] = offset of float i inside transform t of the 16-row image, -1 = padding */
int64_t sf_flow_packed16h_size(const sf_flow* f);
int sf_flow_pack_table16h(const sf_flow* f, int32_t* src, int64_t n);
/* cooperative 16-row training image (MAF, num_blocks 2, D <= 8; csrc/sf_layout.h SfTrcDev): sizes (0 when the flow has
 * none), gather table, logical parameter -> gradient-partial index, and the descriptor as int32 words in declaration order */
int64_t sf_flow_trainc_size(const sf_flow* f);
int64_t sf_flow_trainc_grad_size(const sf_flow* f);
int sf_flow_trainc_table(const sf_flow* f, int32_t* src1, int32_t* src2, int64_t n, int32_t* gdst, int64_t n_params,
                         int32_t* desc /*[64]*/, float* cst, int64_t n_cst);
int64_t sf_flow_cst_size(const sf_flow* f);
/* which kernel sf_flow_loss_grad* runs for a batch of B rows: 0 = one producer wave per 32-sample tile (k_maf_train /
 * k_nsf_train), 1 / 2 = the cooperative 16-row MAF kernel with 4-wave / 8-wave workgroups (k_maf_trainc), 3 = the
 * cooperative 16-row NSF kernel (k_nsf_trainc) */
int sf_flow_train_path(const sf_flow* f, int64_t B, int want_dctx);
/* byte-for-byte description of the packed image for diagnostics (JSON, NUL-terminated) */
int sf_flow_describe(const sf_flow* f, char* buf, size_t buflen);

/* ---- density direction --------------------------------------------------------------
 * out[b] = log N(z;0,I) + sum log|det J|  for theta[b,:], x[b,:]   (raw estimator density)
 * Replaces: flow.log_prob(theta, context=x) (custom_runner.py:604, 646). */
int sf_flow_log_prob(sf_flow* f, const float* theta /*[B,D]*/, const float* x /*[B,C]*/,
                     int64_t B, float* out /*[B]*/, void* stream);

/* ---- posterior mode ------------------------------------------------------------------
 * lp[b] = log q(theta[b] | x[b / rows_per_x]);  dtheta[b, :] = d lp[b] / d theta[b, :]   (raw estimator density, fp32)
 * x is [ceil(B / rows_per_x), C]: rows_per_x consecutive rows of theta share one context row (rows_per_x = 1: aligned
 * rows).  lp or dtheta may be NULL (dtheta NULL: the forward half only).
 * Kinds: SF_MAF and the coupling SF_NSF with D >= 2; the one-parameter NSF and SF_NSF_AR / SF_MAF_AR return
 * SF_ERR_INVALID with a message that names the kind.
 * The backward products read a transposed operand image of the handle's OWN parameter vector: it is built on the first
 * gradient call after sf_flow_set_params and kept until the next sf_flow_set_params.  After sf_flow_loss_grad* /
 * sf_flow_train_epoch* the handle holds no vector of its own and the call returns SF_ERR_STATE, as sf_flow_get_params does:
 * call sf_flow_set_params first.  sf_flow_log_prob, the samplers and training do not see that image.
 * Replaces: the potential's autograd gradient inside DirectPosterior.map -> gradient_ascent [UPSTREAM sbi]. */
int sf_flow_log_prob_grad(sf_flow* f, const float* theta /*[B,D]*/, const float* x, int64_t rows_per_x, int64_t B,
                          float* lp /*[B]*/, float* dtheta /*[B,D]*/, void* stream);

/* One fused ascent step of the mode search for B independent candidates (no handle: elementwise).
 *   theta[b,:]  in: the point at which lp[b] and g_theta[b,:] were evaluated; out: the next point
 *   phi         unconstrained coordinates, theta = lo + (hi - lo) * sigmoid(phi); lo / hi NULL (both): theta = phi
 *   a candidate whose lp or gradient is not finite is frozen: nothing of it is written
 *   save_best != 0 and lp[b] > best_lp[b] (strictly): best_lp[b] = lp[b], best_theta[b,:] = theta[b,:] (the input point)
 *   then torch.optim.Adam's update of phi for the loss -lp (betas 0.9 / 0.999, eps 1e-8, no weight decay, bias
 *   correction for the 1-based `step`) with g_phi = g_theta * (hi - lo) * s * (1 - s)
 *   g_theta NULL: score only (the evaluation after the last step); phi and the moments are not read then.
 * For an ensemble, lp / g_theta are the already combined mixture values. */
int sf_map_step(int64_t B, int64_t D, float* phi /*[B,D]*/, float* exp_avg /*[B,D]*/, float* exp_avg_sq /*[B,D]*/,
                float* theta /*[B,D]*/, const float* lp /*[B]*/, const float* g_theta /*[B,D]*/, const float* lo /*[D]*/,
                const float* hi /*[D]*/, float* best_theta /*[B,D]*/, float* best_lp /*[B]*/, float learning_rate,
                int64_t step, int save_best, void* stream);

/* ---- conditional posteriors: one half-step of the ensemble sampler --------------------
 * The affine-invariant stretch move (Goodman & Weare 2010; emcee's default move) for N independent catalogue rows x W
 * walkers, some coordinates of a row held fixed (no handle: the density is the caller's, evaluated between two launches).
 * One launch does, per row and in this order:
 *   resolve != 0  the pending proposals prop[i] of half-step `half_step - 1`, given their log-density lp_prop[i]: walker w
 *                 takes its proposal iff it lies inside [lo, hi], lp_prop is finite and
 *                 log u < (n_i - 1) log z + lp_prop - lp[i, w]; lp and accepted[i] (+= accepted moves) follow
 *   collect >= 0  walkers[i] and lp[i] are copied to slots collect * W + w of out[i] / out_lp[i] (slots >= S dropped)
 *   propose != 0  the active walkers w % 2 == half_step % 2 write prop[i, w / 2, :] = theta_j + z (theta_w - theta_j) on the
 *                 free coordinates (fixed ones: theta_w copied), partner j = 2 * (((r0 >> 9) * (W / 2)) >> 23) + 1 - h of the
 *                 other half, z = (u + 1)^2 / 2
 * with r = philox4x32_10((p_lo, p_hi, half_step, w), (seed_lo, seed_hi ^ 0x53545200)), p = row_offset + i, u = the uniform
 * of r1 (z) and of r2 (accept), as in the sampler's stream.  The first call of a chain has resolve = 0 and half_step = 0, the
 * last one propose = 0.
 *   fixed[i]   bit d set: coordinate d of row i is fixed (n_i = D minus the set bits); negative: the row is skipped whole
 *              (nothing of it is read or written: a NaN row of the caller)
 *   max_fixed  the caller's bound on the set bits of any row; max_fixed >= D (an empty free set) is refused, and a row that
 *              breaks the bound is skipped
 *   W          even, 4 <= W <= 64;  D in 1..16;  lo / hi NULL (both): no box;  out_lp, trace_* may be NULL
 *   trace_partner / trace_accept [N, W/2]: the partner of every proposal written / the flag of every proposal resolved
 * Replaces: one Python chain per object behind sbi.analysis.conditional_potential + an MCMC posterior [UPSTREAM sbi]. */
int sf_stretch_step(int64_t N, int64_t D, int64_t W, int64_t max_fixed, float* walkers /*[N,W,D]*/, float* lp /*[N,W]*/,
                    const int32_t* fixed /*[N]*/, const float* lo /*[D]*/, const float* hi /*[D]*/,
                    const float* lp_prop /*[N,W/2]*/, float* prop /*[N,W/2,D]*/, int32_t* accepted /*[N]*/,
                    float* out /*[N,S,D]*/, float* out_lp /*[N,S]*/, int64_t S, int64_t collect, uint64_t seed,
                    int64_t row_offset, int64_t half_step, int resolve, int propose, int32_t* trace_partner,
                    int32_t* trace_accept, void* stream);

/* ---- sampling direction -------------------------------------------------------------
 * Parity hook: theta = inverse(z | x), logdet = log|det d theta / d z|  (may be NULL). */
int sf_flow_inverse_from_noise(sf_flow* f, const float* z /*[B,D]*/, const float* x /*[B,C]*/,
                               int64_t B, float* theta /*[B,D]*/, float* logdet /*[B]*/,
                               void* stream);
/* Parity hook of the SAMPLER's arithmetic: the same inverse from given noise, evaluated by the pass functions the
 * persistent sampler (sf_flow_sample) runs in the current mode (sf_set_sampler_fp32).  Returns which arithmetic that was
 * (negative: error):
 *   0  split-bf16 x3 hidden blocks with fp32 accumulation (the opt-in mode of a MAF with H <= 64; the default of the coupling NSF)
 *   1  the generic all-fp32 path (the result is sf_flow_inverse_from_noise's)
 *   2  the 16-row fp32 kernels, both layers of block 0 as they are stored (span placements, and shapes without the fused form)
 *   3  the 16-row fp32 kernels with the first block layer folded into the input layer (W' = W1 W0; the default of a MAF)
 * Replaces nothing in the reference: test surface of posterior.sample's numerics (sbi_runner.py:6442). */
int sf_flow_inverse_from_noise_sampler(sf_flow* f, const float* z /*[B,D]*/, const float* x /*[B,C]*/, int64_t B,
                                       float* theta /*[B,D]*/, void* stream);
/* Arithmetic of the persistent sampler's hidden blocks, process-wide (also: environment SF_SAMPLER_FP32):
 *    1  fp32 everywhere;  0  split-bf16 x3 hidden blocks where the flow has them;
 *   -1  the per-kind default (round 5): fp32 for a MAF -- configs[1] says fp32, and log p of a draw moved by up to 1.3e-3
 *       under the split -- , split for the coupling NSF.  Returns 0. */
int sf_set_sampler_fp32(int on);

/* One rejection round over a list of output slots (slot = g*S + p).  For every listed slot the
 * attempts attempt .. attempt+attempts_per_slot-1 are evaluated together (attempts_per_slot a power
 * of two <= 32) and the LOWEST accepted one is kept, so the result is the same as trying them one
 * after the other:
 *   noise = Philox4x32-10(seed, stream_id; slot, attempt)  ->  theta = inverse(noise | x[g])
 *   accepted (finite and lo <= theta <= hi on every dim; lo/hi NULL = accept all finite):
 *        theta written to out[slot*D ...]
 *   rejected: slot appended to rejected[] (order unspecified), *n_rejected incremented.
 * slots == NULL means the dense list slot = slot_base + i, i < n_slots.
 * n_drawn (may be NULL) [M] int32: += attempts consumed (up to and including the accepted one) for
 * galaxy g, in rounds with attempt > 0 (round 0 is accounted for by the caller: S per galaxy).
 * Replaces: DirectPosterior.sample -> accept_reject_sample (sbi_runner.py:6442; box
 * predicate custom_runner.py:982-987). */
int sf_flow_sample_round(sf_flow* f, const float* x /*[M,C]*/, int64_t S,
                         const uint32_t* slots, int64_t slot_base, int64_t n_slots,
                         uint32_t attempt, int32_t attempts_per_slot, uint64_t seed, uint32_t stream_id,
                         const float* lo /*[D]*/, const float* hi /*[D]*/,
                         float* out /*[M*S, D]*/, uint32_t* rejected, uint32_t* n_rejected,
                         int32_t* n_drawn, void* stream);

/* Optional, for callers that drive the rounds themselves: evaluate everything that depends on a context row
 * alone (the conditioner's context products; in the reference they are recomputed for every one of the S draws
 * of a galaxy inside DirectPosterior.sample, sbi_runner.py:6442) once per row of x[0..M), into a table owned by
 * the handle.  Later sf_flow_sample_round calls that pass the SAME x pointer read the table instead; x must not
 * change until sf_flow_release_context (or the next prepare / set_params / loss_grad, which drop the table).
 * Purely an optimisation: same noise stream, draws equal up to fp32 summation order.  Tables above SF_CTAB_MAX_MB (default
 * 4096) are not built.  sf_flow_sample and sf_flow_acceptance do this internally. */
int sf_flow_prepare_context(sf_flow* f, const float* x /*[M,C]*/, int64_t M, void* stream);
int sf_flow_release_context(sf_flow* f);

/* Whole sampler.  ONE persistent launch works the catalogue's M*S output slots -- first attempts and the retries of
 * rejected slots are scheduled on the device (no host round trip per rejection round) -- up to 1024 attempts per slot
 * (all kernels since round 3).  The few slots that are still empty then (their galaxy accepts less than about one draw
 * in a thousand) are continued chip-wide: a "find" launch evaluates a whole range of attempts of every open slot side by
 * side and records the lowest accepted one, a "resolve" launch re-evaluates exactly that attempt and writes the draw.
 * Every slot keeps the LOWEST accepted attempt of its Philox stream (slot, attempt): the draws do not depend on how the
 * work was scheduled.
 *   max_attempts > 0 : hard ceiling; a slot that used max_attempts attempts becomes a NaN row
 *                      (failure convention of ref: sbi_runner.py:6458-6460).
 *   max_attempts <= 0: no ceiling, like [UPSTREAM] accept_reject_sample, which keeps drawing until S draws are kept:
 *                      a slot is retried for as long as its galaxy still gets draws accepted.  Where an attempt window
 *                      ends (1024, 16384, 262144, ...), and once the galaxy's open slots have used 1e5 attempts since
 *                      the last look, the open slots of a galaxy that got NOT ONE draw accepted since then (counted
 *                      from its 64th attempt on) become NaN rows.
 * The host synchronises the stream once per launch pair (one pinned read-back).  n_drawn [M] may be NULL: attempts
 * consumed per galaxy (int32: pinned at 2^31 - 1 once S x attempts would pass it).  *n_unfilled (host): number of NaN slots. */
int sf_flow_sample(sf_flow* f, const float* x /*[M,C]*/, int64_t M, int64_t S,
                   const float* lo, const float* hi, uint64_t seed, int32_t max_attempts,
                   float* out /*[M,S,D]*/, int32_t* n_drawn /*[M]*/, int64_t* n_unfilled /*host*/,
                   void* stream);

/* Row offset of the NEXT sampling calls on this handle (sf_flow_sample, sf_flow_sample_slots, sf_flow_sample_round,
 * sf_flow_acceptance): the rows passed are rows [row_offset, row_offset + M) of a larger catalogue.  Only the random
 * streams see it (Philox counter = (row_offset + g) * S + p): a chunk of a catalogue, or one rank's contiguous shard of it
 * (rows sharded over GPUs, no collective), then draws exactly what those rows draw in ONE call over the whole
 * catalogue with the same seed.  Stays in force until changed; 0 after sf_flow_create.
 * Replaces: nothing in the reference (its per-galaxy loop, sbi_runner.py:6438-6442, has no batching to be independent of). */
int sf_flow_set_sample_row_offset(sf_flow* f, int64_t row_offset);
/* Output dtype of the next sf_flow_sample / sf_flow_sample_slots calls on this handle: on != 0 -- `out` is a DOUBLE array
 * [M,S,D] (passed through the float* parameter) and every accepted draw is widened fp32 -> float64 in its store (exact).
 * float64 is the container dtype of the reference's sample_posterior (sbi_runner.py:6436: np.zeros((N, S, D))); `out` may be
 * PINNED HOST memory mapped into the device's address space (hipHostMalloc): the draws then cross PCIe while the sampler
 * runs and the reference's host array is complete when the stream is -- no D2H copy and no widening pass afterwards
 * (measured on the cfg2 catalogue: +0.3 ms on a 2.6 ms launch against 1.0 ms for copy + widening).  Not offered for the
 * one-parameter / autoregressive NSF (fp32 + sf_copy_to_host_f64 there). */
int sf_flow_set_sample_output_f64(sf_flow* f, int on);
/* Wall-clock ceiling of later sf_flow_sample / sf_flow_sample_slots calls on this handle (seconds; <= 0 = none, the
 * default): once it is exceeded no further attempt window is opened and the slots still empty become NaN rows.
 * Replaces: the per-object timeout of sample_posterior (timeout_seconds_per_test, ref: sbi_runner.py:6358, 6443-6452). */
int sf_flow_set_sample_time_limit(sf_flow* f, double seconds);

/* The same over an explicit list of output slots (slot = g*S + p; DEVICE uint32 [n_slots], each slot once): only those
 * slots of out are written.  This is what an ensemble member runs on its share of every row's draws
 * ([UPSTREAM] sbi EnsemblePosterior.sample, built at ref: custom_runner.py:278-283). */
int sf_flow_sample_slots(sf_flow* f, const float* x /*[M,C]*/, int64_t M, int64_t S,
                         const uint32_t* slots, int64_t n_slots, const float* lo, const float* hi, uint64_t seed,
                         int32_t max_attempts, float* out /*[M,S,D]*/, int64_t* n_unfilled /*host*/, void* stream);

/* Figures of the last sf_flow_sample / sf_flow_sample_slots call (host [4]): duration in ms of its first persistent
 * launch (HIP events on the call's stream; the only launch unless some slot needed more than 1024 attempts), number of
 * launches, slots whose FIRST attempt was rejected, flow evaluations over all launches. */
int sf_flow_sample_stats(const sf_flow* f, float* stats4);

/* Accepted fraction of n unconstrained draws per row (stream_id 1): count[g] of n.
 * Replaces: DirectPosterior.leakage_correction (custom_runner.py:466-473). */
int sf_flow_acceptance(sf_flow* f, const float* x /*[M,C]*/, int64_t M, int64_t n,
                       const float* lo, const float* hi, uint64_t seed,
                       int32_t* count /*[M]*/, void* stream);

/* ---- training -----------------------------------------------------------------------
 * Forward + backward of  loss_b = -log_prob(theta_b | x_b)  with the parameters given in
 * `flat` (device, logical layout):
 *   loss[b] = loss_b                       (may be NULL)
 *   grad[i] = sum_b w * d loss_b / d flat[i], w = grad_scale (pass 1/B for the mean loss)
 * grad is overwritten (not accumulated).
 * Replaces: train_losses = -estimator.log_prob(...); mean().backward()
 * (custom_runner.py:604-610). */
int sf_flow_loss_grad(sf_flow* f, const float* flat /*[P]*/, const float* theta, const float* x,
                      int64_t B, float grad_scale, float* loss /*[B]*/, float* grad /*[P]*/,
                      void* stream);

/* Same, with the mini-batch gather fused into the kernel: batch row b reads theta[rows[b],:] / x[rows[b],:] of the
 * training arrays (rows: DEVICE int64 [B]); loss / dctx stay batch-indexed.  loss_sum (may be NULL): DEVICE double,
 * += sum_b (-log p_b), the epoch loss accumulator of custom_runner.py:608-611 without a per-step reduction. */
int sf_flow_loss_grad_rows(sf_flow* f, const float* flat, const float* theta /*[N,D]*/, const float* x /*[N,C]*/,
                           const int64_t* rows /*[B]*/, int64_t B, float grad_scale, const float* weights,
                           float* loss, double* loss_sum, float* grad, float* dctx, void* stream);


/* Same with per-sample weights: grad[i] = sum_b grad_scale * weights[b] * d loss_b / d flat[i]
 * (weights NULL = all ones).  This is the vector-Jacobian product torch.autograd needs for an
 * arbitrary reduction of the per-sample losses.
 * dctx (may be NULL) [B,C]: overwritten with grad_scale * weights[b] * d loss_b / d x[b,:] -- the
 * gradient reaching the context, i.e. what an embedding net in front of the flow back-propagates
 * (embedding_net kwarg, ref: sbi_runner.py:4432, custom_runner.py:321). */
int sf_flow_loss_grad_weighted(sf_flow* f, const float* flat, const float* theta, const float* x,
                               int64_t B, float grad_scale, const float* weights /*[B]*/,
                               float* loss, float* grad, float* dctx /*[B,C]*/, void* stream);

/* Measurement hook (bench.py's roofline_train): with profiling on, every sf_flow_loss_grad* call brackets its
 * forward+backward flow kernel with HIP events on the call's stream; sf_flow_train_stats waits for the last such call
 * and returns that kernel's duration in ms.  Off by default (two event records per step are not free at batch 64). */
int sf_flow_set_profiling(sf_flow* f, int on);
int sf_flow_train_stats(sf_flow* f, float* kernel_ms /*host*/);

/* Fused global-norm clip + Adam / AdamW step on flat vectors.
 * Replaces: clip_grad_norm_(max_norm) + optimizer.step() (custom_runner.py:613-618). */
typedef struct sf_adam_desc {
  float lr, beta1, beta2, eps, weight_decay; /* torch defaults 1e-3, .9, .999, 1e-8, 0 (AdamW .01) */
  int32_t decoupled;                           /* 0 = Adam (L2 in grad), 1 = AdamW */
} sf_adam_desc;
int sf_opt_create(int64_t n, const sf_adam_desc* d, sf_opt** out);
void sf_opt_destroy(sf_opt* o);
/* max_norm <= 0 disables clipping; *grad_norm_out (device float, may be NULL) gets the
 * pre-clip global L2 norm.  The norm is summed in a fixed order at every n: the same inputs give
 * the same bits, here and in sf_adam_apply. */
int sf_adam_step(sf_opt* o, float* params, const float* grad, float max_norm,
                 float* grad_norm_out, void* stream);
/* Stateless form: the caller owns exp_avg / exp_avg_sq [n] (device) and the step counter (the
 * value AFTER this update, >= 1).  scratch: 2 device floats; scratch[1] receives the pre-clip
 * global L2 norm.  This is the form the Python runner uses so that optimizer state lives in
 * torch tensors and checkpoints like the reference's (custom_runner.py:693-704). */
int sf_adam_apply(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                  const sf_adam_desc* d, int64_t step, float max_norm, float* scratch, void* stream);

/* One training epoch on a single device without returning to the host between steps
 * (ref: the batch loop of custom_runner.py:585-618): for b < n_batches:
 *   rows = order[b*batch .. (b+1)*batch);  grad = d/dflat sum_rows grad_scale * (-log p);  clip + Adam(W) step
 *   number step0 + b + 1 on flat (state exp_avg / exp_avg_sq, scratch [2] as in sf_adam_apply).
 * order: DEVICE int64 [n_batches*batch] (the epoch's shuffled training rows); grad: DEVICE scratch [P].
 * What the handle represents afterwards: every image (density, samplers, context products) is that of `flat` as it was when the
 * LAST step's gradient was taken, i.e. BEFORE the last update -- the start vector for n_batches = 1.  Between the steps of a call
 * only the training image follows `flat`; the last step re-tiles all of them, and they agree among themselves.  `flat` as returned
 * is one update ahead: to evaluate or sample at it, call sf_flow_set_params(flat) first.  As after sf_flow_loss_grad*, the
 * handle holds no vector of its own (sf_flow_get_params / sf_flow_log_prob_grad: SF_ERR_STATE) and a prepared context table is
 * dropped.  n_batches = 0 leaves the handle as it was. */
int sf_flow_train_epoch(sf_flow* f, float* flat, const float* theta, const float* x, const int64_t* order,
                        int64_t n_batches, int64_t batch, float grad_scale, float* exp_avg, float* exp_avg_sq,
                        const sf_adam_desc* d, int64_t step0, float max_norm, float* scratch /*[2]*/,
                        float* grad /*[P]*/, double* loss_sum, void* stream);

/* ---- data-parallel training: the gradient exchange --------------------------------
 * One process per GPU; every rank holds the same parameters and optimiser state and its own shard of the training rows.
 * Per optimiser step ONE sum all-reduce of the flat fp32 gradient (P floats: 129 KB for the cfg1 MAF) over RCCL -- xGMI
 * inside a node -- on the caller's stream, between the gradient gather and clip + Adam, so that the clip norm and the
 * update are those of the GLOBAL batch on every rank (grad_scale = 1 / (batch x ranks)).
 * Replaces nothing in the reference, which trains on CPU threads only (examples/sbi/slurm/train_final_model.slurm:26): the
 * call sits between `loss.backward()` and `optimizer.step()` of custom_runner.py:585-618.
 * RCCL is bound at run time (dlopen): sf_comm_set_library(path) before the first sf_comm_* call (or the environment variable
 * SF_RCCL_LIB) names the library -- a host that runs PyTorch passes torch's own librccl.so so that the process holds ONE
 * RCCL --, otherwise an already loaded librccl is used, then the loader's search path, then /opt/rocm/lib.
 * Bootstrap as in NCCL: rank 0 calls sf_comm_unique_id, the host ships the SF_COMM_ID_BYTES to every rank by its own means
 * (the torch.distributed store, MPI, a file), every rank calls sf_comm_create (collective) with its HIP device current. */
#define SF_COMM_ID_BYTES 128
typedef struct sf_comm sf_comm;
int sf_comm_set_library(const char* path);
int sf_comm_library(char* path_out, int64_t cap, int* version_out);    /* what was bound (loads it if necessary) */
int sf_comm_unique_id(void* id_out, int64_t bytes);
int sf_comm_create(const void* id, int64_t bytes, int nranks, int rank, sf_comm** out);
void sf_comm_destroy(sf_comm* c);
int sf_comm_info(const sf_comm* c, int* nranks, int* rank);
int sf_comm_all_reduce_sum(sf_comm* c, float* buf /*[n], in place*/, int64_t n, void* stream);
/* sf_flow_train_epoch with the exchange inside: per step  rows -> grad (this rank's shard, grad_scale = 1 / (batch x ranks))
 * -> all-reduce(SUM) over `comm` -> clip + Adam(W), all on `stream`, no host round trip per step.  `order` holds THIS rank's
 * rows; every rank must call it with the same n_batches.  loss_sum stays rank-local (the host reduces it once per epoch with
 * the validation sums, custom_runner.py:655-660).  comm == NULL is sf_flow_train_epoch. */
int sf_flow_train_epoch_dp(sf_flow* f, float* flat, const float* theta, const float* x, const int64_t* order,
                           int64_t n_batches, int64_t batch, float grad_scale, float* exp_avg, float* exp_avg_sq,
                           const sf_adam_desc* d, int64_t step0, float max_norm, float* scratch /*[2]*/,
                           float* grad /*[P]*/, double* loss_sum, sf_comm* comm, void* stream);
/* optimizer state access for checkpoints (custom_runner.py:693-704): exp_avg, exp_avg_sq
 * device pointers [n] and the step counter. */
int sf_opt_state(sf_opt* o, float** exp_avg, float** exp_avg_sq, int64_t** step_host);

/* ---- embedding MLP (context path) ---------------------------------------------------------
 * The optional fully connected embedding net in front of the flow ([UPSTREAM] ili FCN(n_hidden,
 * act_fn="SiLU"): Linear -> act -> ... -> Linear, no activation after the last layer; mentioned at
 * ref: examples/sbi/scripts/train_spectral_model.py:316-317, passed as the embedding_net kwarg,
 * ref: sbi_runner.py:4432).  Flat parameter layout: per layer W[out,in] row-major then b[out]. */
typedef struct sf_mlp sf_mlp;
enum sf_act { SF_ACT_SILU = 0, SF_ACT_RELU = 1, SF_ACT_TANH = 2 };
typedef struct sf_mlp_desc {
  int32_t n_in;        /* input width, 1..512 */
  int32_t n_layers;    /* 1..4 */
  int32_t widths[4];   /* output width of each layer, 1..128 */
  int32_t act;         /* sf_act */
  const float* x_mean; /* host [n_in] or NULL: inputs are standardised as (x - mean)/std in-kernel */
  const float* x_std;  /* host [n_in] or NULL */
} sf_mlp_desc;
int sf_mlp_create(const sf_mlp_desc* d, sf_mlp** out);
void sf_mlp_destroy(sf_mlp* m);
int64_t sf_mlp_num_params(const sf_mlp* m);
/* out[b,:] = MLP(x[b,:]) with the parameters in `flat` (device) */
int sf_mlp_forward(sf_mlp* m, const float* flat, const float* x /*[B,n_in]*/, int64_t B,
                   float* out /*[B,n_out]*/, void* stream);
/* grad[i] = sum_b dout[b,:] . d out[b,:] / d flat[i]   (overwritten) */
int sf_mlp_backward(sf_mlp* m, const float* flat, const float* x, const float* dout /*[B,n_out]*/,
                    int64_t B, float* grad /*[P]*/, void* stream);

/* ---- posterior summaries on the device ---------------------------------------------------
 * out[g,d,k] = quantile q[k] (numpy 'linear' rule) of samples[g,:,d], NaN draws ignored (all NaN -> NaN).
 * Replaces np.quantile(samples_i, quantiles, axis=1) of fit_catalogue (ref: sbi_runner.py:3270-3282)
 * without moving the (N,S,D) draws to the host.  q: DEVICE [Q]; 1 <= S <= 8192.
 * n counts every non-NaN draw, +-inf included (ordered values); the position (n - 1) q and the interpolation are formed in
 * fp64 from the float32 q as given; at an integer position the result is that order statistic bit for bit (also beside an
 * infinite draw).  q is not validated here: for q outside [0, 1] the lower rank is clamped to [0, n - 1] and the end segment
 * extrapolated (defined, not meaningful), a NaN q gives NaN; the Python wrappers refuse both.  sf_quantiles_large: the same. */
int sf_quantiles(const float* samples /*[N,S,D]*/, int64_t N, int64_t S, int32_t D,
                 const float* q /*[Q]*/, int32_t Q, float* out /*[N,D,Q]*/, void* stream);
/* The same contract for long rows, 1 <= S <= 2^24 (the pooled nmc x nposterior draws of the missing-band path, ref:
 * sbi_runner.py:3292-3297): an exact radix select of the order statistics on the draws' bit patterns instead of a sort in
 * LDS; the position (n - 1) q and the interpolation are formed in fp64. */
int sf_quantiles_large(const float* samples /*[N,S,D]*/, int64_t N, int64_t S, int32_t D,
                       const float* q /*[Q]*/, int32_t Q, float* out /*[N,D,Q]*/, void* stream);

/* ---- feature transform on the device ------------------------------------------------------
 * mag = -2.5 log10(flux_nJy / 1000) + 23.9 ; negative flux -> mag_limit ; mag > mag_limit -> mag_limit ; NaN flux -> NaN
 * optional: mag_err = 2.5 err / (ln 10 flux) exactly as the reference computes it (inf for flux == 0, negative for
 * negative flux: the reference does not special-case them either).  All buffers [n] device, 16-byte aligned; err / mag_err may be NULL.
 * Replaces the numpy pass at ref: sbi_runner.py:1698-1716 (AB branch) and 1927-1932 (faint limit). */
int sf_flux_to_abmag(const float* flux_njy, const float* err_njy, int64_t n, float mag_limit,
                     float* mag, float* mag_err, void* stream);

/* asinh magnitudes with per-band softening f_b [C] (nJy, device): flux / err [N,C] row-major in nJy.
 *   mag = -2.5 log10(e) (asinh(f / 2 f_b) + ln(f_b / 3631 Jy)),  mag_err = 2.5 log10(e) err / sqrt(f^2 + (2 f_b)^2)
 * Replaces ref: utils.py:647-704 (f_jy_to_asinh, f_jy_err_to_asinh) as used at sbi_runner.py:1718-1731. */
int sf_flux_to_asinh(const float* flux_njy, const float* err_njy, int64_t N, int32_t C, const float* f_b_njy /*[C]*/,
                     float* mag, float* mag_err, void* stream);

/* Depth-noise scatter of library photometry: out[(i*n_scatters + s), c] = flux[i,c] + sigma_ic * N(0,1),
 * sigma_ic = max(sigma[c], |flux[i,c]| * min_flux_pc_error / 100); err_out (may be NULL) receives sigma_ic.
 * sigma [n_sigma_rows, C] device = depth / depth_sigma in the units of flux; n_sigma_rows = 1 (one depth per band)
 * or n_scatters (a depth set chosen per band and scatter copy: the reference's 2-D depths, the choice is the caller's).
 * Noise from the Philox stream (seed, stream 2).  Replaces ref: sbi_runner.py:580-691 (_apply_depths). */
int sf_scatter_depths(const float* flux /*[N,C]*/, int64_t N, int32_t C, const float* sigma, int32_t n_sigma_rows,
                      int32_t n_scatters, float min_flux_pc_error, uint64_t seed,
                      float* out /*[N*n_scatters,C]*/, float* err_out, void* stream);

/* ---- empirical noise models (csrc/sf_noise.hip; fitted and packed by synference_amd/noise_models.py) ---------------------
 * One band of a packed model: p(sigma | flux) of one filter as three tables over n_bins ascending centres -- centers[n],
 * median[n], std[n] at table[table_offset ...] -- and everything that is constant per band, computed on the host.
 * Spaces: PHYSICAL = a flux density in some unit, AB = AB magnitudes, ASINH = asinh magnitudes with softening b_jy.
 * A physical unit u enters through its AB zero point zp (m = zp - 2.5 log10(f_u); 8.9 for Jy) and through plain factors.
 * Field order and types are mirrored by the ctypes Structure of the same name (synference_amd/_lib.py). */
#define SF_NOISE_KIND_GENERAL 0    /* ref: noise_models.py:638-1099 GeneralEmpiricalUncertaintyModel */
#define SF_NOISE_KIND_ASINH 1      /* ref: noise_models.py:443-635 AsinhEmpiricalUncertaintyModel */
#define SF_NOISE_SPACE_PHYSICAL 0
#define SF_NOISE_SPACE_AB 1
#define SF_NOISE_SPACE_ASINH 2
#define SF_NOISE_FLUX_SCATTER 0    /* limit_value + std_at_limit * N(0,1) truncated to +-3 (unscattered in the scalings call) */
#define SF_NOISE_FLUX_LIMIT 1      /* limit_value */
#define SF_NOISE_FLUX_NUMBER 2     /* flux_number */
typedef struct sf_noise_band {
  int32_t kind;            /* SF_NOISE_KIND_* */
  int32_t interp_space;    /* space of the tables: General PHYSICAL / AB, Asinh ASINH / PHYSICAL */
  int32_t in_space;        /* space of the input flux: PHYSICAL / AB */
  int32_t out_space;       /* General PHYSICAL / AB, Asinh always ASINH */
  int32_t n_bins;          /* 2 .. 256 */
  int32_t table_offset;    /* floats into the table: centers[n_bins], median[n_bins], std[n_bins] */
  int32_t extrapolate;     /* continue the end segments instead of holding the end values */
  int32_t resample;        /* the returned error is a second sigma draw at the scattered flux */
  int32_t upper_limits;    /* General: SNR cut before the scatter */
  int32_t has_limit;       /* General: upper_limit_value exists (SNR cut after the scatter, flux and error rules) */
  int32_t flux_rule;       /* SF_NOISE_FLUX_* */
  int32_t replace_err;     /* the error rule is a recognised one: limited elements get err_value */
  float in_to_unit;        /* physical input -> interpolation unit */
  float zp_in;             /* AB zero point of the physical input unit */
  float zp_unit;           /* AB zero point of the interpolation unit */
  float zp_out;            /* AB zero point of the physical output unit */
  float unit_to_out;       /* interpolation unit -> physical output unit */
  float in_to_jy;          /* physical input -> Jy (Asinh) */
  float unit_per_jy;       /* Jy -> interpolation unit (Asinh, physical tables) */
  float jy_per_unit;       /* interpolation unit -> Jy (Asinh, physical tables) */
  float b_jy;              /* Asinh: softening in Jy */
  float sigma_clip;        /* General: scatter noise truncated to +- this many sigma; negative: not truncated */
  float snr_threshold;     /* treat_as_upper_limits_below */
  float limit_value;       /* upper_limit_value, interpolation space */
  float flux_number;       /* numeric upper_limit_flux_behaviour */
  float std_at_limit;      /* max(0, std table at limit_value) */
  float err_value;         /* the replacement error, interpolation space */
  float min_err;           /* clip of the returned error, output space */
  float max_err;
} sf_noise_band;

/* Scatter every library row n_scatters times through its band's model: out / err_out [(i*n_scatters + s), c] = the noisy flux
 * or magnitude and its error in the band's output space, row order as sf_scatter_depths.  flux [N,C] device in each band's
 * input space; bands [C] and table [n_table] HOST arrays (copied to the device by the call); err_out may be NULL.
 * One Philox4x32-10 call per output element: key (seed, stream 6), counter (out_row lo, out_row hi, 0, band), u0..u3 = the four
 * words as uniforms ((r >> 9) + 0.5) 2^-23.  With x the flux in the band's interpolation space:
 *   sigma(x, u) = mu + ss t,  mu / ss = the median / max(0, std) table at x (linear; NaN in, NaN out),
 *                 t = quantile u of N(0,1) truncated to [a, inf), a = min(-mu / (ss > 1e-9 ? ss : 1), 12)
 *   General: s1 = sigma(x, u0); lim0 = upper_limits and SNR(x, s1) below the threshold or not finite; y = x, and unless lim0
 *     y += s1 z, z the quantile u1 of N(0,1) (truncated to +-sigma_clip); s = resample ? sigma(y, u2) : s1; with has_limit,
 *     where lim0 or SNR(y, s) is below: y by flux_rule (u3), s = err_value; then units out and clip to [min_err, max_err].
 *     SNR in AB space is 2.5 / (ln 10 e) (NaN where the flux is 0 or NaN), in physical space f / e.
 *   Asinh: tables over asinh magnitudes m: s1 = sigma(m, u0), y = m + s1 z, s = resample ? sigma(y, u2) : s1; tables over a
 *     physical unit: s1 = sigma(x, u0), y_jy = f_jy + s1_jy z, y = asinh magnitude of y_jy, e = resample ? sigma(y_jy, u2) : s1,
 *     s = 2.5 log10(e) e_jy / sqrt(y_jy^2 + 4 b^2); then clip.
 * Packed tables above 64 KiB (or structs and tables together above the 64 KiB staged per workgroup), a band with fewer than
 * 2 or more than 256 bins, C < 1: SF_ERR_INVALID with a message, nothing launched.  N == 0: SF_OK, nothing launched.
 * Replaces ref: noise_models.py:818-957 and 507-560 as called from sbi_runner.py:813-903. */
int sf_scatter_empirical(const float* flux /*[N,C] device*/, int64_t N, int32_t C, const sf_noise_band* bands /*[C] host*/,
                         const float* table /*[n_table] host*/, int64_t n_table, int32_t n_scatters, uint64_t seed,
                         float* out /*[N*n_scatters,C] device*/, float* err_out /*device, may be NULL*/, void* stream);

/* The deterministic twin for an observed catalogue (flux, err [N,C] device in each band's input space): units in, SNR cut
 * with the flux rule unscattered, replacement error, units out, clip.  No random numbers.  Same limits as above.
 * Replaces ref: noise_models.py:1074-1099 and 562-592 as called from sbi_runner.py:2767-2843. */
int sf_apply_scalings(const float* flux, const float* err, int64_t N, int32_t C, const sf_noise_band* bands /*[C] host*/,
                      const float* table /*[n_table] host*/, int64_t n_table, float* out, float* err_out, void* stream);

/* ---- spectral libraries: observed-frame spectra features (csrc/sf_spectra.hip; driven by synference_amd/spectra.py) ------
 * Every pointer is a DEVICE pointer; the struct itself is read on the host.  Field order and types are mirrored by the ctypes
 * Structure of the same name (synference_amd/_lib.py).  Per row i of flux [N, ld_flux] on the ascending grid wave[L] (um):
 *   SF_SPECTRA_TRANSFORM (ref: utils.py:185-254): wz = wave (1 + z[i]); sigma = sqrt(max(s_inst^2 - s_th^2, 0)) / pix in fp64,
 *     s_inst = wz / interp(wz, curve_wave, curve_r) / 2 sqrt(2 ln 2), s_th the same with theory_r (theory_r_arr[L] when not
 *     NULL), pix = the median of diff(wz) = the mean of the differences at med_lo and med_hi (the host names the middle one
 *     or two); the variable-width Gaussian (sigma <= 0.01: copied; else weights exp(-x^2 / 2 sigma^2), |x| <= ceil(trunc sigma),
 *     divided by their sum, indices clamped to the row); then SpectRes with fill 0 onto observed_wave[M]; the flux is not
 *     divided by 1 + z.  out [N, ld_out], M values per row.
 *   SF_SPECTRA_CONVOLVE (ref: utils.py:129-182): the Gaussian alone with sigma_pixels[i * sigma_stride + .] (stride 0: one
 *     row for all); out holds L values per row, no normalisation, units or clip.
 *   SF_SPECTRA_UNITS: nothing is convolved or rebinned; out[i, j] = flux[i, col0 + j], j < M, through the steps below.
 *   A pixel whose half-width exceeds h_limit, or whose sigma is NaN, comes out NaN: h_limit bounds the tap loop.
 * Normalisation (ref: sbi_runner.py:1096-1178): tophat and bandpass are both a linear functional of the spectrum, so the
 * host hands over its coefficients: the factor is sum(flux norm_table[L]) over the raw row (SF_SPECTRA_NORM_REST, and either
 * frame in SF_SPECTRA_UNITS, where the reference normalises on the uncropped theory grid too) or sum(bins norm_table[M])
 * over the rebinned row (SF_SPECTRA_NORM_OBSERVED); the row is divided by it, a factor of 0 gives a row of 0.
 * Units and clip (ref: 1361-1381): LINEAR v unit_scale; LOG10 log10(v unit_scale); AB -2.5 log10(v unit_scale) + 8.9 with
 * unit_scale = Jy per grid unit (negative flux NaN, zero +inf); then clipped to [clip_lo, clip_hi], NaN kept.
 * SF_ERR_INVALID with a message and nothing launched: L above SF_SPECTRA_MAX_L (two float arrays of L in LDS) unless
 * SF_SPECTRA_UNITS, a curve above SF_SPECTRA_MAX_CURVE nodes, fewer than 2 pixels on a grid that needs bin edges, h_limit
 * outside 1 .. SF_SPECTRA_MAX_HALF_WIDTH, a stride shorter than its row.  N == 0: SF_OK.  Asynchronous on `stream`. */
#define SF_SPECTRA_UNITS 0
#define SF_SPECTRA_TRANSFORM 1
#define SF_SPECTRA_CONVOLVE 2
#define SF_SPECTRA_NORM_NONE 0
#define SF_SPECTRA_NORM_REST 1
#define SF_SPECTRA_NORM_OBSERVED 2
#define SF_SPECTRA_UNIT_LINEAR 0
#define SF_SPECTRA_UNIT_LOG10 1
#define SF_SPECTRA_UNIT_AB 2
#define SF_SPECTRA_MAX_L 16384
#define SF_SPECTRA_MAX_CURVE 256
#define SF_SPECTRA_MAX_HALF_WIDTH 65536
typedef struct sf_spectra_desc {
  const float* flux;            /* [N, ld_flux] */
  const double* wave;           /* [L] um, ascending */
  const double* z;              /* [N]; TRANSFORM only */
  const double* sigma_pixels;   /* CONVOLVE only */
  const double* observed_wave;  /* [M] um, ascending; TRANSFORM only */
  const double* curve_wave;     /* [n_curve] um, ascending */
  const double* curve_r;        /* [n_curve] */
  const double* theory_r_arr;   /* [L] or NULL: then theory_r */
  const double* norm_table;     /* [L] or [M]; NULL with SF_SPECTRA_NORM_NONE */
  float* out;                   /* [N, ld_out] */
  int64_t N, ld_flux, ld_out, sigma_stride;
  int32_t mode;                 /* SF_SPECTRA_UNITS / TRANSFORM / CONVOLVE */
  int32_t L, M, n_curve;
  int32_t col0;                 /* UNITS: first kept column */
  int32_t norm_frame;           /* SF_SPECTRA_NORM_* */
  int32_t unit_code;            /* SF_SPECTRA_UNIT_* */
  int32_t med_lo, med_hi;       /* TRANSFORM: the middle difference(s) of diff(wave) */
  int32_t h_limit;
  double theory_r;              /* may be inf */
  double trunc;
  float unit_scale, clip_lo, clip_hi;
} sf_spectra_desc;
int sf_spectra_transform(const sf_spectra_desc* desc, void* stream);

/* PIT ranks of the truths among the posterior draws: out[g,d] = #{draws < truth} / #{non-NaN draws}
 * (NaN when there are none; +-inf draws are ordered values and count on both sides; a NaN truth gives 0).
 * Replaces the host pass at ref: sbi_runner.py:7153-7158. */
int sf_pit_ranks(const float* samples /*[N,S,D]*/, const float* truth /*[N,D]*/, int64_t N, int64_t S, int32_t D,
                 float* out /*[N,D]*/, void* stream);

/* TARP expected-coverage curves (Lemos et al. 2023, "Sampling-Based Accuracy Testing of Posterior Estimators"), restated from
 * the paper -- the reference calls the third-party `tarp` package: get_tarp_coverage(samples, y, norm=True, bootstrap=True,
 * num_bootstrap=200).  Per pass b over a row list idx[b,:] and reference points r[b,j,:], with i = idx[b,j]:
 *   counts[b,j] = #{ s : dist(r, samples[i,s,:]) < dist(r, theta[i,:]) }   (a NaN draw compares false and stays in S)
 *   ecp[b,e]    = #{ j : counts[b,j] / S < edges[e] } / N  (ecp[b,0] = 0, ecp[b,bins] = 1), edges = np.histogram's:
 *                 linspace(min f, max f, bins + 1), min - 0.5 / max + 0.5 when they are equal.
 * norm_axis >= 0: draws and truths become (v - low) / (high - low + 1e-10), low / high the min / max of the pass's resampled
 * truths over the positions (0: per parameter) or over the parameters (1: per position).  num_bootstrap = B > 0: B passes,
 * idx[b,j] = (uint64(r0) * N) >> 32 from Philox (seed, stream 3; counter (j, 0, b, 0)); 0: one pass over the rows in order.
 * references NULL: r[b,j,d] uniform in [0,1) from Philox (seed, stream 4; counter (j, 0, b, d / 4)), else row j in every pass.
 * 1 <= D <= 16, 1 <= S <= 8192, N >= 1, num_alpha_bins >= 1, max(B,1) * N < 2^31.  The draws are read from HBM once per call;
 * the counts are exact integers, so two calls give the same bits.
 * Replaces ref: sbi_runner.py:7090-7126 (calculate_TARP) and 6618-6637 (the `tarp` key of evaluate_model). */
int sf_tarp_coverage(const float* samples /*[N,S,D] device*/, const float* theta /*[N,D] device*/,
                     int64_t N, int64_t S, int32_t D,
                     const float* references /*[N,D] device, or NULL: Philox stream 4*/,
                     int32_t metric /*0 euclidean, 1 manhattan*/, int32_t norm_axis /*-1 no normalisation, 0, 1*/,
                     int32_t num_bootstrap /*0: one pass over the rows in order*/, int32_t num_alpha_bins, uint64_t seed,
                     double* ecp /*[max(B,1), bins+1] device*/, double* alpha /*[bins+1] device, last pass; may be NULL*/,
                     int32_t* counts /*[max(B,1), N] device; may be NULL*/, int32_t* boot_idx /*[B,N] device, out; may be NULL*/,
                     void* stream);

/* SBI++ missing-band imputation (ref: sbi_runner.py:7736-7791 _get_neighbor_kdes / _chi2dof, 7831-7841 generate_imputations,
 * Mode 1; the KDE is scipy.stats.gaussian_kde in one dimension with bw_method = bw and weights).  Per object m, V its observed
 * bands and X its missing ones:
 *   chi2[t] = (sum_{b in V} ((train[t,band_col[b]] - obs[m,band_col[b]]) / sigma[m,b])^2) / dof in fp32, every operation
 *     rounded on its own, NaN terms skipped, dof = the finite observed values among V;
 *   thresholds ini_chi2, ini_chi2 + chi2_step, ... <= max_chi2 (fp32 sums, at most 32): the first that admits at least
 *     min_neighbours rows; none: the rows under the last one; no row at all: the fallback_k rows of smallest chi2 (ties to the
 *     lowest row); a final set below min_neighbours is a failure: n_used = -1 (-2: no finite observed band), NaN outputs;
 *   w = 1 / dist, dist the fp64 Euclidean distance over V (0 -> 1e-10); var_b = bw^2 sum wn (x - mu)^2 / (1 - sum wn^2), fp64;
 *   draw (i, b in X): r = Philox(counter ((row_offset + m) lo, hi, i, b), key (seed, stream 5)); neighbour = the first j, in
 *     ascending training row, whose running fp64 weight sum exceeds (r0 + 0.5) 2^-32 times the total; value = x_j + sqrt(var) z,
 *     z the first normal of (r2, r3) of the sampler's Box-Muller.
 * imputed[m,i,:] = obs[m,:] with the column of every missing band replaced by its draw and, with err_col, its error column by
 * the drawn neighbour's own error value; recon[m,b] = mean over i for missing bands, NaN for observed ones.
 * 1 <= B <= 32, B <= F <= 64, NT < 2^31.  Exact and reproducible: integer counts, ordered lists, fixed summation order; the
 * draws of an object do not depend on how the objects are split over calls.  Scratch is owned per device; the neighbour lists
 * of a group of objects stay within SF_IMPUTE_SCRATCH_BYTES [256 MiB] (one object alone may exceed it).  The call waits on
 * `stream` once per batch of objects (it reads the list lengths back to form the groups). */
int sf_impute_missing(const float* train /*[NT,F] device*/, int64_t NT, int32_t F,
                      const int32_t* band_col /*[B] host*/, const int32_t* err_col /*[B] host, or NULL*/, int32_t B,
                      const float* obs /*[M,F] device*/, const float* sigma /*[M,B] device*/,
                      const uint8_t* missing /*[M,B] device, 1 = missing*/, int64_t M, int64_t row_offset,
                      float ini_chi2, float chi2_step, float max_chi2, int32_t min_neighbours, int32_t fallback_k, float bw,
                      int32_t nmc, uint64_t seed,
                      float* imputed /*[M,nmc,F] device*/, float* recon /*[M,B] device*/,
                      int32_t* n_used /*[M] device: neighbours used, or a negative failure code*/,
                      float* thr_used /*[M] device, may be NULL: the threshold used (the last one tried on failure / fallback)*/,
                      double* kde_var /*[M,B] device, may be NULL: NaN for observed bands*/,
                      int32_t* nbr_idx /*[M,nbr_cap] device, may be NULL: the first nbr_cap neighbours, ascending row*/,
                      int64_t nbr_cap,
                      int32_t* draw_idx /*[M,nmc,B] device, may be NULL: training row drawn, -1 for observed bands*/,
                      void* stream);

/* ---- out-of-distribution check: the all-pairs kernels (csrc/sf_ood.hip; synference_amd/ood.py builds LOF, kNN and KDE scores
 * on them -- ref: utils.py:991-1340 detect_outliers / detect_outliers_pyod, sbi_runner.py:3777-3945 test_in_distribution) -----
 * Squared distance of two rows, everywhere: acc = 0; for c ascending: t = q[c] - b[c]; acc = acc + t * t, every operation
 * rounded to nearest in fp32 and none fused.  A NaN distance (a NaN in the base row) counts as +inf.
 *
 * sf_knn: the k nearest rows of base[N,C] for every row of query[M,C], exact and brute force.  Candidates order by
 * (d2 bits, base row): equal distances go to the lowest row, so the result is ONE set: it does not depend on chunking, on
 * tiling or on how the queries are split over calls.  exclude_self = 1: base row self_offset + m is not a neighbour of query m
 * (the base against itself, possibly in pieces).  Outputs ascending.  1 <= C <= 64, 1 <= k <= 64, k <= N - exclude_self,
 * N < 2^31, with exclude_self self_offset + M <= N; anything else is SF_ERR_INVALID and the outputs are untouched.
 * Asynchronous on `stream`; scratch (M x splits x k keys when few queries meet a long base) is owned per device. */
int sf_knn(const float* base /*[N,C] device*/, int64_t N, int32_t C, const float* query /*[M,C] device*/, int64_t M,
           int32_t k, int32_t exclude_self, int64_t self_offset,
           float* d2 /*[M,k] device, ascending*/, int32_t* idx /*[M,k] device*/, void* stream);

/* out[m] = log sum_i exp(-d2(query_w[m], base_w[i]) / 2) over rows that the caller has whitened (scipy.stats.gaussian_kde's
 * and pyod KDE's kernel sum without the normalisation).  Terms are v_exp_f32 of the distance above the running minimum, added
 * in fp64 in ascending row order per split of the base, the splits in ascending order; the split count depends on the shapes
 * alone: two calls give the same bits.  No finite distance: -inf.  1 <= C <= 64, N < 2^31. */
int sf_kde_logsumexp(const float* base_w /*[N,C] device*/, int64_t N, int32_t C, const float* query_w /*[M,C] device*/,
                     int64_t M, double* out /*[M] device*/, void* stream);

/* ---- Gaussian-kernel sums of the MMD misspecification test (csrc/sf_mmd.hip; synference_amd/misspecification.py; DESIGN.md
 * section 18).  A term is k(a, b) = exp2(d2(a, b) * c2) with d2 the squared distance above (fp32, unfused), the product rounded
 * to fp32 and v_exp_f32; c2 = (float)(-0.5 / scale^2 * log2(e)) comes from the caller, c2 <= 0 and finite.  A NaN term counts
 * as 0.  Sums are fp64 of fp32 terms in an order fixed by the shapes alone -- no atomics: two calls give the same bits.
 *
 * sf_rbf_rowsum: out[q] = sum_i k(query[q], base[i]); exclude_self = 1 skips base row self_offset + q (by position, as in
 * sf_knn: the base against itself, possibly in pieces).  1 <= C <= SF_RBF_MAX_C, 1 <= N < 2^31, with exclude_self
 * self_offset + M <= N; anything else is SF_ERR_INVALID with a message and the output is untouched.  M == 0: SF_OK. */
#define SF_RBF_MAX_C 64
int sf_rbf_rowsum(const float* base /*[N,C] device*/, int64_t N, int32_t C, const float* query /*[M,C] device*/, int64_t M,
                  float c2, int32_t exclude_self, int64_t self_offset, double* out /*[M] device*/, void* stream);

/* sf_rbf_subset_sums: pair_sum[s] = sum over positions a != b of k(rows[idx[s,a]], rows[idx[s,b]]) -- ordered pairs, the
 * exclusion by position -- and, with rowsum, picked_rowsum[s] = sum_a rowsum[idx[s,a]].  Only the tiles on and below the
 * diagonal of the m x m block are visited; terms below it are doubled.  The entries of a set being distinct and inside [0, N)
 * is the caller's contract; the device clamps an entry outside into the range and never reads out of bounds.
 * 1 <= C <= SF_RBF_MAX_C, N < 2^31, 2 <= m <= N, rowsum and picked_rowsum both NULL or both given; anything else is
 * SF_ERR_INVALID with a message and the outputs are untouched.  n_sets == 0: SF_OK.  Scratch (one partial per visited tile of
 * at most 64 MiB of sets at a time) is owned per device. */
int sf_rbf_subset_sums(const float* rows /*[N,C] device*/, int64_t N, int32_t C, const int32_t* idx /*[n_sets,m] device*/,
                       int64_t n_sets, int64_t m, float c2, const double* rowsum /*[N] device or NULL*/,
                       double* pair_sum /*[n_sets] device*/, double* picked_rowsum /*[n_sets] device; NULL iff rowsum NULL*/,
                       void* stream);

/* ---- L-C2ST: the classifiers of the local calibration test (csrc/sf_lc2st.hip; synference_amd/lc2st.py; DESIGN.md section 15;
 * ref: sbi_runner.py:986-1063, sbi.diagnostics.lc2st.LC2ST with sklearn's MLPClassifier) ---------------------------------------
 * A handle holds n_cls independent classifiers over ONE row matrix rows[R, n_in]: two ReLU layers of `width` units and a logistic
 * output, Adam on the mean binary cross-entropy plus alpha / (2 n) |W|^2, minibatches of `batch` rows (the last one shorter) in a
 * fresh keyed order every epoch, the validation accuracy after every epoch, sklearn's stopping rule when early_stopping is set
 * (count of epochs with score < best + tol; stop when it exceeds n_iter_no_change; the best-score weights are the result).
 * Classifier c trains on the rows with vmask[c][r] == 0 against labels[c][r] (0 / 1) and is scored on the rows with vmask 1.
 * A parameter vector is sklearn's, dense and row major: W1[n_in][width], b1[width], W2[width][width], b2[width], w3[width], b3.
 * The order of epoch e of classifier c: position j visits training row number F(j), F a four-round Feistel bijection walked
 * into [0, n_train), its round keys philox4x32_10((c, e, 0, 0), (seed_lo, seed_hi ^ 0x4C433200)) (lc2st.keyed_order).
 * rows and labels are read by every later call and stay the caller's; vmask and init_weights are consumed by create.
 * 1 <= n_in <= SF_C2ST_MAX_IN, 1 <= width <= SF_C2ST_MAX_W, 1 <= R < 2^31: anything else is SF_ERR_INVALID with a message that
 * names the limit; no device: SF_ERR_NO_DEVICE. */
#define SF_C2ST_MAX_IN 80
#define SF_C2ST_MAX_W 128
typedef struct sf_c2st sf_c2st;
typedef struct {
  int32_t n_in, width, n_cls, max_iter, n_iter_no_change, early_stopping, batch;
  int64_t R;
  uint64_t seed;
  float lr, beta1, beta2, eps, alpha;
  double tol;
  const float* rows;          /* [R, n_in] device */
  const uint8_t* labels;      /* [n_cls, R] device */
  const uint8_t* vmask;       /* [n_cls, R] device */
  const float* init_weights;  /* [n_cls, num_params] device */
} sf_c2st_desc;
int sf_c2st_create(const sf_c2st_desc* desc, sf_c2st** out, void* stream);
void sf_c2st_destroy(sf_c2st* h);
int64_t sf_c2st_num_params(const sf_c2st* h);
/* One launch: classifiers first .. first + count - 1, one workgroup each, run up to `epochs` more epochs from the state the
 * handle keeps (weights, Adam moments and step, best snapshot, counters) and stop early by the rule or at max_iter.  finish != 0
 * ends the classifiers of the range where they stand (the best snapshot becomes the result).  Blocking; *n_active: classifiers
 * of the range not yet done.  The result does not depend on how the epochs are split over launches. */
int sf_c2st_train(sf_c2st* h, int32_t first, int32_t count, int32_t epochs, int32_t finish, int32_t* n_active, void* stream);
/* rows_o[S, n_in]: stats[i] = mean_s (p - 0.5)^2 (fp64, ascending s) with p = 1 - sigmoid(logit) of classifier first + i;
 * probs[i, s] = p when probs is not NULL.  Asynchronous on `stream`. */
int sf_c2st_scores(sf_c2st* h, int32_t first, int32_t count, const float* rows_o /*device*/, int64_t S,
                   double* stats /*[count] device*/, float* probs /*[count,S] device or NULL*/, void* stream);
/* To HOST arrays, each may be NULL: weights[n_cls, num_params]; score_log[n_cls, max_iter], the correct validation rows after
 * each epoch (-1: epoch not run); state[n_cls, 8] = n_iter, Adam steps, no-improvement count, best_iter, done, n_train, n_val,
 * best count.  Blocking. */
int sf_c2st_get(sf_c2st* h, float* weights, int32_t* score_log, int32_t* state, void* stream);

/* ---- hand-over to the host ----------------------------------------------------------------
 * host_dst[i] = (double) dev_src[i], i < n: the draws of a catalogue call leave HBM as fp32 in pieces through a ring of pinned
 * staging buffers on a private copy stream and are widened into the caller's float64 array (any host memory, not necessarily
 * pinned) by a pool of host threads with streaming stores, copy and widening overlapped.  Work queued on `stream` before the
 * call is waited for; blocking; one call at a time per process.  SF_HOSTIO_PIECE_MB [4], SF_HOSTIO_THREADS [min(8, cgroup
 * CPU quota)].
 * Replaces: `samples[i] = posterior.sample(...).detach().cpu().numpy()` into the float64 array (sbi_runner.py:6436-6457). */
int sf_copy_to_host_f64(const float* dev_src /*device [n]*/, double* host_dst /*host [n]*/, int64_t n, void* stream);


/* ---- misc --------------------------------------------------------------------------- */
const char* sf_last_error(void);
const char* sf_version(void);
/* number of visible HIP devices (0 on a CPU-only box; never fails) */
int sf_device_count(void);

/* ---- latents -------------------------------------------------------------------------
 * The density direction with its latent handed out ([UPSTREAM] nflows Flow.transform_to_noise): z = T(theta; x) in the column
 * order sf_flow_inverse_from_noise reads, logabsdet = log |det dz / dtheta| with the standardisation term, so that
 * sf_flow_log_prob = -0.5 |z|^2 - 0.5 D log(2 pi) + logabsdet.  The same kernels as sf_flow_log_prob; either output may be
 * NULL; B == 0 is a no-op.  Asynchronous on `stream`. */
int sf_flow_to_noise(sf_flow* f, const float* theta /*[B,D]*/, const float* x /*[B,C]*/, int64_t B,
                     float* z /*[B,D] or NULL*/, float* logabsdet /*[B] or NULL*/, void* stream);
/* One pass over z[N, D] (1 <= D <= 16, N >= 0), every output a device array that may be NULL.  A row counts if all its D values
 * are finite (n), the others are skipped (n_bad).  psum[p, d] = sum z_d^(p+1), cross[i, j] = sum z_i z_j, both accumulated in
 * fp64; pit_counts[d, b]: rows with min(floor(u nb), nb - 1) == b for u = Phi(z_d) = 0.5 erfc(-z_d / sqrt 2);
 * radial_counts[b]: the same for u = F_chi2_D(|z|^2) (both in fp64; 1 <= nb <= 1024).  Deterministic: two calls give the same
 * bits.  Asynchronous on `stream`. */
int sf_latent_summary(const float* z /*[N,D] device*/, int64_t N, int32_t D, int32_t nb,
                      int64_t* n2 /*[2]: n, n_bad*/, double* psum /*[4,D]*/, double* cross /*[D,D]*/,
                      int64_t* pit_counts /*[D,nb]*/, int64_t* radial_counts /*[nb]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SYNFERENCE_HIP_H */
