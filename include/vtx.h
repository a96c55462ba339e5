/* vtx.h -- C ABI of libvtx.so: hand-written gfx950 (MI355X / CDNA4) kernels for the ViT / Swin
 * training hot path of rosinality/vision-transformers-pytorch.
 *
 * The reference has no FFI layer: its boundary is the Python nn.Module surface (SURVEY.md
 * section 8(b)).  These entry points are what the MI355X-native nn.Modules in
 * vision-transformers-pytorch_amd/models/ call (through ctypes, vtx/_lib.py) in place of the stock
 * PyTorch op compositions of the reference; each declaration cites the reference lines it replaces.
 *
 * Conventions (all entry points):
 *   - return 0 on success, a negative VTX_ERR_* code otherwise (vtx_strerror); never throw, never exit
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch caching allocator), including
 *     workspaces whose size comes from the matching vtx_*_workspace(); no ownership transfer
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*) and never synchronise; re-entrant across
 *     streams / threads (autograd's backward thread).  Process-global mutable state, all of it DIAGNOSTIC: (1) the table
 *     of dispatch switches behind vtx_set_option (atomic ints, read once per call: a switch flipped while another thread
 *     is inside an entry point takes effect at that thread's next call); (2) the launch timer of vtx_timer_start /
 *     vtx_timer_stop (csrc/layer.hip: one unsynchronised record list -- while a timer is open, vtx_layer_* / vtx_srlayer_*
 *     calls append to it from whichever thread enqueues them, so open it only around single-threaded, single-stream
 *     sections: bench.py's event-sampled steps; with no timer open the layer calls touch no shared state)
 *   - dtype: VTX_F32 (parity mode, exact-fp32 MFMA) or VTX_BF16 (training mode: bf16 storage,
 *     fp32 accumulation / statistics); parameters, their gradients and all statistics are fp32
 *   - activations are row-major [rows, C] (tokens x channels) = NHWC / (B, L, C)
 */
#ifndef VTX_H_
#define VTX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VTX_F32 0
#define VTX_BF16 1

#define VTX_OK 0
#define VTX_ERR_SHAPE (-1)
#define VTX_ERR_DTYPE (-2)
#define VTX_ERR_ALIGN (-3)
#define VTX_ERR_LAUNCH (-4)
#define VTX_ERR_WORKSPACE (-5)
#define VTX_ERR_NULL (-6)
#define VTX_ERR_JPEG (-7)      /* not a supported JPEG (the reason is in VtxJpegInfo.reason), or an invalid decode plan */

const char* vtx_strerror(int code);
/* ABI version of the library (bumped on any signature change): what this header declares, and what vtx_abi_version() of a
 * library compiled against it returns.  vtx/_lib.py binds the library from this file and refuses one of another version. */
#define VTX_ABI_VERSION 30
int vtx_abi_version(void);
/* Compute units of the current device (256 on MI355X; 256 when no device can be asked): what the one-workgroup-per-CU kernels size their
 * grids and the dispatch heuristics their thresholds with.  The heuristics themselves live in the library only: the bindings ask
 * vtx_gemm_route / vtx_wgrad_route / vtx_wattn_route (below) which kernel a launch takes. */
int vtx_cu_count(void);
/* Test helper: fill the LDS of every CU with `pattern` (160-KB workgroups, `rounds` per CU): LDS is not cleared between workgroups, and a
 * kernel that reads LDS it never wrote sees what the previous workgroup left there (tests/test_gpu_lds_poison.py). */
int vtx_debug_lds_poison(unsigned pattern, int rounds, void* stream);
/* Measurement helper (bench.py `measured_peaks`, SURVEY.md section 8(d): "ideally a measured MFMA micro-benchmark on the box"): one launch of
 * waves_per_cu / 4 256-thread workgroups per CU (waves_per_cu in 4, 8, .. 32), every wave issuing 4 * iters dense bf16 MFMAs
 * (v_mfma_f32_32x32x16_bf16, 32 768 FLOP each) on register operands, no memory traffic.  *flops receives the FLOPs of the launch; the caller
 * brackets the call with events on `stream`.  `sink`: any device buffer of >= 4 bytes. */
int vtx_debug_mfma_peak(int iters, int waves_per_cu, void* sink, double* flops, void* stream);
/* Measurement helper: one idle wavefront that occupies `stream` for `microseconds` of wall clock (<= 100 000) and touches no memory.  Two of
 * them on two streams finish in one period when the streams run concurrently, in two when they share a hardware queue: vtx.functional picks
 * the side stream of the weight gradients with it (round 6, profiles/round6_side_stream_queue.md). */
int vtx_debug_spin(int microseconds, void* stream);
/* waves per workgroup the ViT attention fast path (csrc/attention_seq.hip) runs sequences of L tokens with under the current SATTN_WAVES option
 * (round 6: 6 / 7 / 8 so that the live 16-token tiles divide among the waves; the bindings name the kernel instantiation with it) */
int vtx_sattn_waves(int L);

/* ---- Dispatch switches (csrc/options.h).  Which kernel variant an entry point launches -- LDS-DMA vs register-staged
 * GEMM, tile height, waves per workgroup, split-K target, fused vs separate split-K reduction, persistent-grid sizes --
 * is a table of ints, initialised from the environment variable of the same name (vtx_option_name: "VTX_GLDS_BM", ...)
 * at library load and changeable in-process: every variant computes the same function (most of them bit-identically,
 * tests/test_gpu_dispatch.py), the switches exist for measurement and for parity tests at a forced dispatch.
 * (The reference has no counterpart: its dispatch is torch's.) */
int vtx_option_count(void);
const char* vtx_option_name(int id);
int vtx_get_option(int id);              /* -1 for an unknown id */
int vtx_set_option(int id, int value);   /* VTX_ERR_SHAPE for an unknown id */

/* ---- LayerNorm (reference: nn.LayerNorm at models/vit.py:13, models/swin_transformer.py:12,
 * 206, 221, 277).  y = (x - mean) * rstd * gamma + beta over the last dim, biased variance.
 * merge != 0: x is (B, H, W, C/4) NHWC and row (b, i, j) is the 2x2 patchify gather of
 * PatchMerge (models/swin_transformer.py:15-22, 224) -- the 4C-wide row is never materialised.
 * Saves mean / rstd [rows] for the backward. */
int vtx_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                      int64_t rows, int C, float eps, int dtype, int merge, int H, int W, void* stream);
/* Over the kept samples of a stochastic-depth branch only (csrc/layer.hip drives these): logical row r is row
 * perm[r / T] * T + r % T of every row-indexed tensor, perm [samples] int32 on the device with the kept samples first. */
int vtx_layernorm_fwd_mapped(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                             int64_t rows, int C, float eps, int dtype, const int* perm, int T, void* stream);
int vtx_layernorm_bwd_mapped(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                             const void* dres, void* dx, void* workspace, size_t ws_bytes, int64_t rows, int64_t live, int C,
                             int dtype, const int* perm, int T, void* stream);
size_t vtx_layernorm_bwd_workspace(int64_t rows, int C);
/* dx = dres + LN'(dy)  (dres optional, plain layout only), dgamma / dbeta fp32 [C] (overwritten).
 * dgamma == dbeta == NULL defers the final column reduce: the per-block partials stay in the workspace as
 * [vtx_layernorm_bwd_blocks(rows, C)][2 C] fp32 and the caller sums them -- together with the layer's other small
 * reductions -- in one vtx_colreduce_multi launch (same summation order, same bits). */
int vtx_layernorm_bwd_blocks(int64_t rows, int C);
int vtx_colreduce_multi(int n, const float* const* part, float* const* out0, float* const* out1, const int* nb,
                        const int* C, const int* ld, void* stream);
int vtx_layernorm_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                      const void* dres, void* dx, float* dgamma, float* dbeta, void* workspace, size_t ws_bytes,
                      int64_t rows, int C, int dtype, int merge, int H, int W, void* stream);

/* ---- Linear layers (reference: nn.Linear / nn.Conv2d-as-GEMM at models/vit.py:23-25, 73,
 * models/swin_transformer.py:34-35, 205, 222, 281, models/layer.py:191-196) with fused epilogues.
 *   mode 0 (forward): C[M,N] = epi( A[M,K] . B[N,K]^T )        A = activations, B = weight
 *   mode 1 (dgrad)  : C[M,N] = epi( A[M,K] . B[K,N]   )        A = dy, B = weight [K = out, N = in]
 *   epi(v): v += bias[col]; act 1: aux_out = z = v, v = silu(z) (MLP, models/layer.py:191-196);
 *           act 2: v *= silu'(aux_in[row,col]);
 *           v *= rowscale[row / rows_per_scale] (DropPath, models/layer.py:172-180);
 *           v += resid[row, col] (residual add, models/vit.py:60-61, swin_transformer.py:194-195)
 * bias / resid / rowscale / aux_out / aux_in may be NULL.  lda/ldb/ldc in elements; N, K and the leading dimensions
 * must be multiples of 8 (16-byte vector access everywhere). */
int vtx_gemm(int mode, int dtype, const void* A, const void* B, void* C, int M, int N, int K, int64_t lda,
             int64_t ldb, int64_t ldc, const float* bias, const void* resid, const float* rowscale,
             int rows_per_scale, void* aux_out, const void* aux_in, int act, void* stream);
/* ---- Routing queries.  Which kernel instantiation a GEMM, a weight gradient or a window-attention launch takes is decided once, in the
 * library (csrc/gemm.hip gemm_route and its per-family parts, wgrad_group_route, wattn_route), from the shapes, the operands that are
 * present, the dispatch switches and the CU count.  The launchers switch on that decision; these entries return the same decision for a
 * launch described by shape alone, with the name of the instantiation as rocprofv3 prints it (abbreviated as bench.py and the tests know
 * it).  They touch no device memory, launch nothing and work without a GPU.  VtxRoute / VtxGemmQuery: vtx_layer_desc_bytes(4 / 5). */
typedef struct VtxRoute {
  int family;                 /* GEMM: 1 skinny | 2 two-group | 3 A-stationary | 4 LDS-DMA wave-private epilogue | 5 LDS-DMA | 6 register-staged;
                                 weight gradient: 1 LDS-DMA 128 x 128 | 2 wide | 3 register-staged;  window attention: 1 one wave | 2 four waves */
  int tile_m, tile_n, tile_k, stages, waves;   /* tiled families: tile, k-depth, ring stages; waves along N (LDS-DMA) / per workgroup */
  int wmf, nf, ktiles;        /* two-group: tile height / 32 and tile width / 64; k-tiles of skinny (K / 32) and A-stationary (K / 64) */
  int mapped, act, resid, aux;   /* what the instantiation is specialised on (where its family templates on it) */
  int wide_j, tiles;          /* wide weight gradient: tile width / 64 and the tiles of the group */
  int reserved;
  char label[96];
} VtxRoute;
#define VTX_Q_RESID 1         /* (bits 0..3 = the flag bits of a VtxTimerRec) */
#define VTX_Q_AUXOUT 2
#define VTX_Q_AUXIN 4
#define VTX_Q_MAPPED 8
#define VTX_Q_BIAS 16
#define VTX_Q_ROWSCALE 32
#define VTX_Q_INPLACE 64      /* resid == C */
typedef struct VtxGemmQuery {
  int mode, dtype, M, N, K, act;   /* as vtx_gemm; mode 2: the register-staged weight gradient dW[M, N] over K tokens */
  int flags;                  /* VTX_Q_*: the operands that are present (contiguous leading dimensions assumed) */
  int Mk, map_T;              /* VTX_Q_MAPPED: rows computed and rows per sample; map_T == 0: unknown (a timer record) -- one sample of Mk rows */
  int rows_per_scale;         /* with VTX_Q_ROWSCALE (<= 0: 1; a mapped launch: map_T) */
} VtxGemmQuery;
int vtx_gemm_route(const VtxGemmQuery* q, VtxRoute* out);
/* nprob == 1 and flags bit 0 clear: vtx_wgrad (flags bit 1: a rowscale is present);  flags bit 0: the grouped launch (bit 2: row-mapped) */
int vtx_wgrad_route(int dtype, int nprob, const int* N, const int* Kin, int64_t mtok, int flags, int rows_per_scale,
                    float scale_const, VtxRoute* out);
int vtx_wattn_route(int dtype, int bwd, int masked, int problems_per_head, int inverse_map, VtxRoute* out);
/* 1 where the LDS-DMA forward-layout kernels take a [*, K] x [N, K]^T GEMM: a dgrad then runs on the transposed weight copy */
int vtx_gemm_glds_ok(int N, int K);

/* ---- Fused MLP of the narrow stages (csrc/mlp_fused.hip; reference models/layer.py:186-196 inside models/swin_transformer.py:193-197):
 * bf16, C = 64 / 96, ff % 32 == 0, both weights resident in LDS, >= 32 768 rows (vtx_mlp_fused_ok tells; option MLP_FUSED).
 *   vtx_mlp_fwd: y = resid + rowscale[row / rows_per_scale] * (silu(ln2 . w1^T + b1) . w2^T + b2); z (the bf16 pre-activation) and
 *                h = silu(z) are written only when their pointers are given (the one-call layers pass NULL: nothing ff-wide is stored);
 *   vtx_mlp_bwd: z and h recomputed from ln2; dz = rowscale * (dy . w2) * silu'(z) and h written for the weight gradients
 *                (dW2 = dy^T h, dW1 = dz^T ln2: vtx_wgrad_group), dln2 = dz . w1.
 * w1 [ff][C], w2 [C][ff] bf16 (the forward-layout copies); b1 / b2 / resid / rowscale may be NULL.  Element values: those of the
 * four vtx_gemm launches they replace, bit for bit. */
int vtx_mlp_fused_ok(int dtype, int64_t M, int C, int ff);
int vtx_mlp_fwd(int dtype, const void* ln2, const void* w1, const float* b1, const void* w2, const float* b2, const void* resid,
                const float* rowscale, int rows_per_scale, void* y, void* z, void* h, int64_t M, int C, int ff, void* stream);
int vtx_mlp_bwd(int dtype, const void* ln2, const void* dy, const void* w1, const float* b1, const void* w2, const float* rowscale,
                int rows_per_scale, void* h, void* dz, void* dln2, int64_t M, int C, int ff, void* stream);
/*   vtx_mlp_bwd_ln (round 6, option LN_FOLD): vtx_mlp_bwd with the LayerNorm backward of the block's norm_ff (models/swin_transformer.py:196:
 *                out + drop_path(ff(norm_ff(out)))) in its epilogue -- dx1 = dy + LN'(dln2) with LN' over x1 / mean / rstd / gamma, the bits of
 *                vtx_mlp_bwd followed by vtx_layernorm_bwd(dln2, x1, mean, rstd, gamma, dres = dy); dln2 is never stored.  part: the
 *                [part_rows][2 C] fp32 dgamma | dbeta partial rows of vtx_layernorm_bwd's deferred reduce (vtx_colreduce_multi); part_rows >=
 *                vtx_cu_count(): the launch writes one row per workgroup and zeroes the others. */
int vtx_mlp_bwd_ln(int dtype, const void* ln2, const void* dy, const void* w1, const float* b1, const void* w2, const float* rowscale,
                   int rows_per_scale, void* h, void* dz, const void* x1, const float* mean, const float* rstd, const float* gamma,
                   void* dx1, float* part, int part_rows, int64_t M, int C, int ff, void* stream);
/* ---- Narrow-layer input gradient with the LayerNorm backward in its epilogue (round 6, option LN_FOLD bit 1; csrc/gemm_skinny.hip):
 * dx = dres + LN'(dy . W) -- the bits of vtx_gemm(dy [M, K], wt [C, K] = W^T) followed by vtx_layernorm_bwd(dln, x, mean, rstd, gamma,
 * dres); the intermediate dln [M, C] is never stored.  bf16, C in {64, 96, 128}, K = 3 C (a packed qkv projection, reference
 * models/swin_transformer.py:128,194) or K = C.  part: as in vtx_mlp_bwd_ln. */
int vtx_dgrad_ln(int dtype, const void* dy, const void* wt, const void* x, const float* mean, const float* rstd, const float* gamma,
                 const void* dres, void* dx, float* part, int part_rows, int64_t M, int C, int K, void* stream);
/* ---- LayerNorm FORWARD folded into its consumer (round 6, option LN_FOLD bits 2, 3): the norm runs on the row operands of a row-streaming
 * launch (csrc/ln_fold.h); the normalised rows and the statistics are stored on the side for the backward; outputs bit-identical to
 * vtx_layernorm_fwd followed by the consumer.
 *   vtx_mlp_fwd_ln: LN(x1; gamma, beta, eps) -> ln2, mean, rstd;  y = x1 + rowscale * MLP(ln2)      (vtx_layernorm_fwd + vtx_mlp_fwd)
 *   vtx_ln_gemm:    LN(x) -> ln_out, mean, rstd;  y = ln_out . w^T + bias, w [N][C]                   (vtx_layernorm_fwd + vtx_gemm)
 * bf16; C in {64, 96} (MLP) / {64, 96, 128} (GEMM, N % 32 == 0). */
int vtx_mlp_fwd_ln(int dtype, const void* x1, const float* gamma, const float* beta, float eps, void* ln2, float* mean, float* rstd,
                   const void* w1, const float* b1, const void* w2, const float* b2, const float* rowscale, int rows_per_scale, void* y,
                   int64_t M, int C, int ff, void* stream);
int vtx_ln_gemm(int dtype, const void* x, const float* gamma, const float* beta, float eps, void* ln_out, float* mean, float* rstd,
                const void* w, const float* bias, void* y, int64_t M, int C, int N, void* stream);
size_t vtx_wgrad_workspace(int64_t mtok, int N, int Kin);
/* dW[N,Kin] = sum_m s[m] dy[m,:]^T x[m,:] (fp32, overwritten); dbias[N] = sum_m s[m] dy[m,:] (optional,
 * computed inside the same kernel).  s = rowscale[m / rows_per_scale] or 1.  scale_const > 0 declares that
 * every rowscale value is either 0 or scale_const (DropPath: mask / (1 - p)), which lets the LDS-DMA kernel
 * skip dropped samples' rows instead of scaling; pass 0 for arbitrary scales.
 * Deterministic: split-K over tokens into fp32 slabs in `workspace`, summed in slice order by ONE following reduce launch.
 * dW needs 16-byte alignment (the kernels store 16-byte vectors): VTX_ERR_ALIGN otherwise. */
int vtx_wgrad(int dtype, const void* dy, const void* x, float* dW, float* dbias, int64_t mtok, int N, int Kin,
              int64_t ld_dy, int64_t ld_x, const float* rowscale, int rows_per_scale, float scale_const,
              void* workspace, size_t ws_bytes, void* stream);
/* Grouped form: the weight gradients of nprob <= vtx_wgrad_group_max() linears over the SAME mtok tokens in ONE launch
 * -- the four of a transformer layer's backward (fc2, fc1, proj, qkv: models/vit.py:59-63, swin_transformer.py:193-197,
 * layer.py:191-196).  Split-K only exists to fill the chip, so four problems together need a quarter of the slices (and
 * of the fp32 slab traffic) of one.  bf16, every (N[i], Kin[i]) a multiple of 8 and >= 64 (vtx_wgrad_group_ok tells;
 * otherwise call vtx_wgrad per problem).  Arrays are HOST arrays of nprob entries; dbias / rowscale may be NULL or hold
 * NULL entries; rowscale values in {0, scale_const} (scale_const > 0) as for vtx_wgrad; same determinism contract.
 * ncol (0..4) deferred column reductions (the arguments of vtx_colreduce_multi: a layer's LayerNorm dgamma / dbeta partials,
 * its rel_pos gradient partials) ride in the group's ONE reduce launch -- same bits as vtx_colreduce_multi, one launch less
 * per layer.  They must have been enqueued on `stream` (or be ordered before it) like the operands.
 * accumulate != 0 (needs vtx_wgrad_group_slices() >= 2): every output (dW, dbias, col_out0 / 1) becomes out + result -- a
 * parameter's second gradient inside one backward (DINO's multi-crop backbone, train_dino.py:229-236) lands on the first
 * instead of in a tensor of its own that autograd then has to add (one `add` launch per parameter). */
int vtx_wgrad_group_max(void);
int vtx_wgrad_group_ok(int dtype, int nprob, const int* N, const int* Kin, int64_t mtok, int has_rowscale,
                       int rows_per_scale, float scale_const);
size_t vtx_wgrad_group_workspace(int nprob, const int* N, const int* Kin, int64_t mtok);
int vtx_wgrad_group(int dtype, int nprob, const void* const* dy, const void* const* x, float* const* dW,
                    float* const* dbias, const int* N, const int* Kin, const int64_t* ld_dy, const int64_t* ld_x,
                    const float* const* rowscale, int rows_per_scale, float scale_const, int64_t mtok,
                    void* workspace, size_t ws_bytes, int ncol, const float* const* col_part, float* const* col_out0,
                    float* const* col_out1, const int* col_nb, const int* col_C, const int* col_ld, int accumulate,
                    void* stream);
/* ... over the KEPT samples of stochastic-depth branches (csrc/layer.hip drives it): problem i with perm[i] != NULL
 * contracts over the mtok_kept[i] tokens of its kept samples only, in perm[i] order (logical token t = row
 * perm[i][t / rows_per_scale] * rows_per_scale + t % rows_per_scale of dy[i] and x[i]; dropped samples' rows are never read)
 * and multiplies its result by scale[i]; rowscale[i] must be NULL for it.  perm == NULL: exactly vtx_wgrad_group. */
int vtx_wgrad_group_mapped(int dtype, int nprob, const void* const* dy, const void* const* x, float* const* dW,
                           float* const* dbias, const int* N, const int* Kin, const int64_t* ld_dy, const int64_t* ld_x,
                           const float* const* rowscale, const int* const* perm, const int* mtok_kept, const float* scale,
                           int rows_per_scale, float scale_const, int64_t mtok, void* workspace, size_t ws_bytes, int ncol,
                           const float* const* col_part, float* const* col_out0, float* const* col_out1, const int* col_nb,
                           const int* col_C, const int* col_ld, int accumulate, void* stream);
/* split-K slices such a group runs with (>= 2: its outputs come from the reduce launch, so `accumulate` is available) */
int vtx_wgrad_group_slices(int nprob, const int* N, const int* Kin, int64_t mtok);

/* ---- Attention cores.  qkv is the QKV-projection output [rows, 3*nH*D] with channel order
 * [q|k|v][head][d] (models/vit.py:30-34, models/swin_transformer.py:128); o is [rows, nH*D].
 *   swin == 0 (reference models/vit.py:30-42): L tokens per image, rows = B*L.
 *   swin != 0 (reference models/swin_transformer.py:109-154): (H, W) NHWC feature map, win x win
 *     windows (L = win*win), shift != 0 selects the rolled partition (roll by -win/2 and back are
 *     folded into addressing); bias = [nH][L][L] fp32 from vtx_relpos_bias; mask = local_mask
 *     buffer [nW][L][L] bytes (True = -inf) or NULL.
 * lse [B*nW*nH*L] fp32 (log-sum-exp per query row) is saved for the backward.
 * Global attention (swin == 0, no bias / mask) runs at ANY L: up to 224 tokens on the register-resident kernels, beyond
 * (e.g. 577 = ViT-S/16 at 384 x 384, models/vit.py:153-175) on key-block / online-softmax kernels (csrc/attention_long.hip);
 * their backward needs vtx_attention_bwd_workspace() bytes of workspace (B*nH*L floats). */
int vtx_relpos_bias(const float* rel_pos, const int64_t* pos, float* bias, int L, int nH, void* stream);
int vtx_attention_fwd(const void* qkv, void* o, float* lse, const float* bias, const uint8_t* mask, int B, int L,
                      int nH, int D, int swin, int H, int W, int win, int shift, int dtype, void* stream);
size_t vtx_attention_bwd_workspace(int B, int L, int nH, int swin, int H, int W, int win);
/* global attention over Bk <= B images only (the b-th one is image perm[b]; lse indexed by b): bf16, D = 64, L <= 224 */
int vtx_attention_fwd_mapped(const void* qkv, void* o, float* lse, const int* perm, int Bk, int L, int nH, int D, int dtype,
                             void* stream);
int vtx_attention_bwd_mapped(const void* qkv, const void* o, const void* dout, const float* lse, void* dqkv, const int* perm,
                             int Bk, int L, int nH, int D, int dtype, void* stream);
/* dqkv [rows, 3*nH*D] (fully overwritten).  With bias: drel_pos [ntab, nH] fp32 = dense gradient of
 * the rel_pos embedding (models/swin_transformer.py:46,135), scattered through the CSR (order[L*L],
 * offsets[ntab+1]) of the pos table; deterministic (no atomics). */
int vtx_attention_bwd(const void* qkv, const void* o, const void* dout, const float* lse, const float* bias,
                      const uint8_t* mask, const int* csr_order, const int* csr_offsets, void* dqkv,
                      float* drel_pos, int ntab, void* workspace, size_t ws_bytes, int B, int L, int nH, int D,
                      int swin, int H, int W, int win, int shift, int dtype, void* stream);

/* ---- Dropout of the attention probabilities (reference models/vit.py:39, models/swin_transformer.py:144: F.dropout(attn, p,
 * training) on the softmax output; models/pvt.py:60, models/twins.py:88,147 likewise).  Same arguments as vtx_attention_fwd / _bwd
 * plus (drop_p, seed, keep): cell (problem, query, key) is kept when a counter-based hash of (seed, problem, query * L + key) says
 * so -- the backward regenerates the decision from the same (drop_p, seed), no mask tensor exists in HBM -- and kept
 * probabilities are scaled by 1 / (1 - drop_p).  problem = (image * nW + window) * nH + head.  keep != NULL replaces the hash by
 * an explicit mask [problems][L][L] of bytes (1 = keep): the parity tests pass the mask the reference drew.  0 < drop_p < 1.
 * Global attention of any length (key-block kernels beyond 224 tokens); with a window, a bias or a mask the register-resident kernels:
 * <= 160 tokens (head dim 32) or <= 224 tokens (head dim 64), VTX_ERR_SHAPE beyond -- and, with a bias, <= 160 tokens in the backward
 * (the register-resident bias gradient).
 * vtx_attn_keep_mask writes the hash's decisions [nprob][Lq][Lk] (what the kernels regenerate) for tests / an external checker. */
int vtx_attention_fwd_drop(const void* qkv, void* o, float* lse, const float* bias, const uint8_t* mask, int B, int L,
                           int nH, int D, int swin, int H, int W, int win, int shift, int dtype, float drop_p, uint64_t seed,
                           const uint8_t* keep, void* stream);
int vtx_attention_bwd_drop(const void* qkv, const void* o, const void* dout, const float* lse, const float* bias,
                           const uint8_t* mask, const int* csr_order, const int* csr_offsets, void* dqkv,
                           float* drel_pos, int ntab, void* workspace, size_t ws_bytes, int B, int L, int nH, int D,
                           int swin, int H, int W, int win, int shift, int dtype, float drop_p, uint64_t seed,
                           const uint8_t* keep, void* stream);
int vtx_attn_keep_mask(uint8_t* out, int64_t nprob, int Lq, int Lk, float drop_p, uint64_t seed, void* stream);

/* ---- Window attention fast path (head dim 32, window <= 7x7): one wavefront per (image, window, head) problem,
 * persistent 4-wave workgroups per head, same semantics as vtx_attention_fwd/bwd with swin != 0
 * (reference models/swin_transformer.py:103-160: roll, partition, q k^T / sqrt(d) + rel_pos(pos) bias,
 * masked_fill(local_mask, -inf), softmax, @ v, inverse partition, roll back).
 *   rel_pos [(2 win - 1)^2][nH] fp32 (the nn.Embedding weight), pos [L][L] int64 (the module's `pos` buffer);
 *   region: NULL for un-shifted layers, else [nW][64] uint8 with
 *           local_mask[n][a][b] == (region[n][a] != region[n][b])   (swin_transformer.py:82-89, 138-141)
 *           -- vtx.tables.mask_regions derives the ids from the module's local_mask buffer and verifies the
 *           identity; a mask without that structure takes vtx_attention_* instead.
 * The head's bias table is gathered into LDS once per workgroup; no per-call table kernels.
 * The backward writes dqkv fully and drel_pos [(2 win - 1)^2][nH] (deterministic). */
int vtx_wattn_fwd(const void* qkv, void* o, float* lse, const float* rel_pos, const int64_t* pos,
                  const uint8_t* region, int B, int L, int nH, int H, int W, int win, int shift, int dtype,
                  void* stream);
int vtx_wattn_fwd_mapped(const void* qkv, void* o, float* lse, const float* rel_pos, const int64_t* pos,
                         const uint8_t* region, const int* perm, int Bk, int L, int nH, int H, int W, int win, int shift,
                         int dtype, void* stream);     /* the b-th image worked on is image perm[b], b < Bk */
int vtx_wattn_bwd_mapped(const void* qkv, const void* o, const void* dout, const float* lse, const float* rel_pos,
                         const int64_t* pos, const uint8_t* region, void* dqkv, void* workspace, size_t ws_bytes,
                         const int* inv_cells, int inv_count, const int* perm, int Bk, int L, int nH, int H, int W, int win,
                         int shift, int dtype, void* stream);
size_t vtx_wattn_bwd_workspace(int B, int nH, int H, int W, int win);
/* drel_pos == NULL defers the rel_pos-gradient reduce: vtx_wattn_bwd_parts() partial rows of stride vtx_wattn_bwd_part_ld(nH)
 * stay in the workspace (columns (2 win - 1)^2 * nH) for vtx_colreduce_multi. */
int vtx_wattn_bwd_parts(int B, int nH, int H, int W, int win);
int vtx_wattn_bwd_part_ld(int nH);
/* inv_cells [inv_count][(2 win - 1)^2] int32 (device) or NULL: the inverse of pos -- inv_cells[t][b] = the t-th cell
 * q * 64 + key (row stride 64) with pos[q][key] == b in ascending (q, key) order, padded with the cell L * 64; inv_count = the
 * largest bin (vtx.tables.pos_inverse).  With it the rel_pos gradient is gathered per bin inside the kernel; NULL: LDS-atomic
 * scatter (~27 us more per launch, same result up to fp32 summation order). */
int vtx_wattn_bwd(const void* qkv, const void* o, const void* dout, const float* lse, const float* rel_pos,
                  const int64_t* pos, const uint8_t* region, void* dqkv, float* drel_pos, void* workspace,
                  size_t ws_bytes, const int* inv_cells, int inv_count, int B, int L, int nH, int H, int W, int win,
                  int shift, int dtype, void* stream);

/* ---- One call per transformer layer (csrc/layer.hip): the pre-LN block of models/vit.py:59-63 and
 * models/swin_transformer.py:193-197 --  x1 = x + s1 * proj(attn(qkv(LN1 x)));  y = x1 + s2 * fc2(silu(fc1(LN2 x1)))  -- as
 * ONE descriptor: vtx_layer_fwd enqueues the 7 launches, vtx_layer_bwd the 8 + 2 of the backward (the entry points above, in
 * the order vtx.functional.TransformerLayerFn issues them: bit-identical results), so that the host pays one call and one
 * activation buffer per layer instead of ~19 calls and ~28 allocations (host time per Swin-S step 13.9 -> see DESIGN).
 * All pointers are device addresses the caller keeps alive; weights (wq, wo, w1, w2: [out][in]) are in the compute dtype,
 * the transposed copies (w?t: [in][out]) may be NULL (then every dgrad takes the register-staged kernel); s1 / s2 are the
 * per-sample DropPath scales (NULL: none) with values in {0, scale_const}.
 *   attn_kind VTX_ATTN_WINDOW: vtx_wattn_fwd / _bwd (rel_pos, pos, region, H, W, win, shift; B images, L = win^2);
 *             VTX_ATTN_GLOBAL: vtx_attention_fwd / _bwd without bias / mask (B images of L tokens, head dim C / nH).
 * Backward: dz / dln2 / dx1 / dout / dqkv / dln1 are scratch; ln?_ws (vtx_layernorm_bwd_workspace), attn_ws
 * (vtx_wattn_bwd_workspace / vtx_attention_bwd_workspace) and wgrad_ws (vtx_wgrad_group_workspace for the problems
 * (C, ff), (ff, C), (C, C), (3C, C)) are workspaces; dW? / db? / dg? / dbe? (/ drel) receive the parameter gradients (fp32).
 * `side_stream` != NULL sends the grouped weight gradient + its reduce there behind an event fork; the caller joins.
 * accumulate: as for vtx_wgrad_group. */
#define VTX_ATTN_WINDOW 1
#define VTX_ATTN_GLOBAL 2
typedef struct VtxLayerFwd {
  int dtype, attn_kind;
  int64_t M;                                   /* tokens */
  int C, ff, nH, L, B, rows_per_scale;
  int H, W, win, shift;
  float eps;
  const void* x;
  const float *ln1_w, *ln1_b, *ln2_w, *ln2_b;
  const void *wq, *wo, *w1, *w2;
  const float *bq, *bo, *b1, *b2;
  const float* rel_pos; const int64_t* pos; const uint8_t* region;
  const float *s1, *s2;
  void *ln1, *qkv, *o, *x1, *ln2, *z, *h, *y;  /* z may be NULL (no backward will run) */
  float *mean1, *rstd1, *mean2, *rstd2, *lse;
  /* stochastic-depth compaction (both NULL: off): perm1 / perm2 [B] int32 on the device list the samples of the attention /
   * MLP branch, kept ones (s? != 0) first, Bk1 / Bk2 >= 1 of them -- each branch is computed for its kept samples only, the
   * others pass through (bf16; window attention, or global attention with head dim 64 and L <= 224; C and ff multiples of
   * 128; rows_per_scale = tokens per sample) */
  const int *perm1, *perm2;
  int Bk1, Bk2;
} VtxLayerFwd;
int vtx_layer_fwd(const VtxLayerFwd* a, void* stream);
typedef struct VtxLayerBwd {
  int dtype, attn_kind;
  int64_t M;
  int C, ff, nH, L, B, rows_per_scale;
  int H, W, win, shift;
  float scale_const;
  int accumulate, inv_count;
  const void *dy, *x, *ln1, *qkv, *o, *x1, *ln2, *z, *h;
  const float *mean1, *rstd1, *mean2, *rstd2, *lse;
  const float *ln1_w, *ln2_w;
  const void *wq, *wo, *w1, *w2, *wqt, *wot, *w1t, *w2t;
  const float* rel_pos; const int64_t* pos; const uint8_t* region; const int* inv_cells;
  const float *s1, *s2;
  void *dz, *dln2, *dx1, *dout, *dqkv, *dln1, *dx;
  void *ln1_ws, *ln2_ws, *attn_ws, *wgrad_ws;
  size_t ln_ws_bytes, attn_ws_bytes, wgrad_ws_bytes;
  float *dWq, *dbq, *dWo, *dbo, *dW1, *db1, *dW2, *db2, *dg1, *dbe1, *dg2, *dbe2, *drel;
  const int *perm1, *perm2;                    /* the forward's (see VtxLayerFwd) */
  int Bk1, Bk2;
  const float* b1;                             /* fc1 bias: a forward that ran the fused MLP (vtx_mlp_fwd) kept no z -- the backward recomputes it */
} VtxLayerBwd;
int vtx_layer_bwd(const VtxLayerBwd* a, void* stream, void* side_stream);
int vtx_layer_desc_bytes(int which);
/* The same for the layers built around the spatial-reduction (sub-sampled) attention: one PVT block (reference
 * models/pvt.py:31-68, 99-103) or the global half of a Twins-SVT layer (models/twins.py:56-93, 201-202):
 *   x1 = x + s1 * proj(sr_attn(q(LN1 x), kv(reduce(LN1 x))))      y = x1 + s2 * fc2(silu(fc1(LN2 x1)))
 * reduce (r > 1) = operand gather (vtx_patchify_fwd, or vtx_twins_subsample_fwd when twins != 0) + GEMM + bias [+ LayerNorm
 * when srn_w != NULL]; splitk != 0: the reduction conv runs as vtx_wgrad on the transposed operand copy + vtx_bias_cast.
 * r == 1: keys / values come from LN1's output directly (Lk = L).  linear_q / linear_kv have no bias.  The caller owns every
 * buffer; the backward's weight gradients run as two grouped launches (the M-token problems with the LayerNorm column
 * reductions; the B*Lk-token problems of the reduction branch) on `side_stream` when given, like vtx_layer_bwd. */
typedef struct VtxSrLayerFwd {
  int dtype, twins;
  int64_t M;                                   /* B * L tokens */
  int C, ff, nH, L, B, rows_per_scale, H, W, r, skip, Lk, splitk;
  float eps;
  const void* x;
  const float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *srn_w, *srn_b;
  const void *wq, *wkv, *wsr, *wsr_t, *wo, *w1, *w2;
  const float *bsr, *bo, *b1, *b2;
  const float *s1, *s2;
  void *ln1, *q, *patches, *patches_t, *red32, *red, *kvin, *kv, *o, *x1, *ln2, *z, *h, *y;
  float *mean1, *rstd1, *mean2, *rstd2, *means, *rstds, *lse;
  void* splitk_ws;
  size_t splitk_ws_bytes;
} VtxSrLayerFwd;
int vtx_srlayer_fwd(const VtxSrLayerFwd* a, void* stream);
typedef struct VtxSrLayerBwd {
  int dtype, twins;
  int64_t M;
  int C, ff, nH, L, B, rows_per_scale, H, W, r, skip, Lk, reserved;
  float scale_const;
  const void *dy, *x, *ln1, *q, *patches, *red, *kvin, *kv, *o, *x1, *ln2, *z, *h;
  const float *mean1, *rstd1, *mean2, *rstd2, *means, *rstds, *lse;
  const float *ln1_w, *ln2_w, *srn_w;
  const void *wq, *wkv, *wsr, *wo, *w1, *w2, *wqt, *wkvt, *wsrt, *wot, *w1t, *w2t;
  const float *s1, *s2;
  void *dz, *dln2, *dx1, *dout, *dq, *dkv, *dkvin, *dred, *dpatches, *dln1, *dx;
  void *ln1_ws, *ln2_ws, *lns_ws, *attn_ws, *wgrad_ws, *wgrad2_ws;
  size_t ln_ws_bytes, lns_ws_bytes, attn_ws_bytes, wgrad_ws_bytes, wgrad2_ws_bytes;
  float *dWq, *dWkv, *dWsr, *dbsr, *dWo, *dbo, *dW1, *db1, *dW2, *db2, *dg1, *dbe1, *dg2, *dbe2, *dgs, *dbs;
  const float* b1;                             /* fc1 bias (the fused MLP's backward recomputes z: see VtxLayerBwd) */
} VtxSrLayerBwd;
int vtx_srlayer_bwd(const VtxSrLayerBwd* a, void* stream, void* side_stream);
/* sizeof the descriptors: 0 / 1 VtxLayerFwd / Bwd, 2 / 3 VtxSrLayerFwd / Bwd */
/* Per-launch HIP-event timing of what vtx_layer_* enqueues (bench.py's roofline block describes the kernels of the timed
 * path): between vtx_timer_start() and vtx_timer_stop() every launch of a layer call is bracketed by two events on its
 * stream; _stop synchronises and returns up to `cap` records.  tag: VTX_T_*; rows = rows / tokens the launch computes;
 * GEMM: C[rows, n] over k; attention: n heads, k tokens per problem; flags: 1 residual, 2 z written, 4 z read, 8 row-mapped
 * (compacted branch), 16 shifted-window mask. */
enum { VTX_T_LN_FWD = 1, VTX_T_GEMM = 2, VTX_T_WATTN_FWD = 3, VTX_T_ATTN_FWD = 4, VTX_T_LN_BWD = 5, VTX_T_WATTN_BWD = 6,
       VTX_T_ATTN_BWD = 7, VTX_T_WGRAD = 8,
       /* vtx_srlayer_*: sub-sampled attention (rows = B*Lq queries, n heads, k keys); its layer's grouped weight gradients over
        * rows tokens: _SR_A = fc2, fc1, proj, q [, kv when flags & 1] with n = C, k = ff; _SR_B = kv + reduction conv with n = C,
        * k = r*r*C; _SPLITK = ONE problem dW[n, k] over rows tokens (the reduction conv's forward on the split-K launch);
        * _GATHER = operand gather / scatter of rows x n elements */
       VTX_T_SRATTN_FWD = 9, VTX_T_SRATTN_BWD = 10, VTX_T_WGRAD_SR_A = 11, VTX_T_WGRAD_SR_B = 12, VTX_T_WGRAD_SPLITK = 13,
       VTX_T_GATHER = 14,
       /* the fused MLP of the narrow stages (vtx_mlp_fwd / vtx_mlp_bwd inside vtx_layer_*): rows, n = C, k = ff */
       VTX_T_MLP_FWD = 15, VTX_T_MLP_BWD = 16,
       /* round 6: a dgrad with the LayerNorm backward in its epilogue (csrc/gemm_skinny.hip dgrad_ln_kernel): rows x C (n) over k */
       VTX_T_DGRAD_LN = 17,
       /* a LayerNorm forward on the row operands of the GEMM that consumes it (gemm_skinny.hip, LNF): rows x n over k = C */
       VTX_T_LN_GEMM = 18 };
typedef struct VtxTimerRec { int tag, n, k, flags; int64_t rows; float ms; } VtxTimerRec;
int vtx_timer_start(void);
int vtx_timer_stop(VtxTimerRec* out, int cap);   /* sizeof(VtxLayerFwd) (0) / sizeof(VtxLayerBwd) (1), for bindings */

/* ---- Spatial-reduction (cross) attention of PVT (csrc/attention_sr.hip; reference models/pvt.py:38-66) and the global
 * sub-sampled attention of Twins-SVT (models/twins.py:56-93): head dim D = 64 | 32, Lq queries against Lk reduced keys per
 * (image, head): up to 64 keys on the register-resident kernels (every 224 x 224 configuration), more (PVT at 256 x 256 stage 4:
 * 65; at 384 x 384: 144 / 145; Twins at 448 x 448: 256) on key-block / online-softmax kernels (csrc/attention_long.hip).
 *   q [B*Lq, nH*D] (= linear_q output), kv [B*Lk, 2*nH*D] (= linear_kv output: k | v halves, pvt.py:51, twins.py:74),
 *   o [B*Lq, nH*D], lse [B*nH*Lq] fp32 (saved for the backward).
 * The backward writes dq and dkv fully; key-side partials are summed in fixed order (deterministic). */
int vtx_srattn_fwd(const void* q, const void* kv, void* o, float* lse, int B, int Lq, int Lk, int nH, int D, int dtype,
                   void* stream);
/* score [B, nH, Lq, Lk] = q k^T / sqrt(D) before the softmax: the second value pvt.MultiHeadedAttention.forward returns
 * (models/pvt.py:53, 69; the PVT layers discard it).  Inference-side helper: no backward. */
int vtx_srattn_scores(const void* q, const void* kv, void* score, int B, int Lq, int Lk, int nH, int D, int dtype,
                      void* stream);
size_t vtx_srattn_bwd_workspace(int B, int Lq, int Lk, int nH, int D);
int vtx_srattn_bwd(const void* q, const void* kv, const void* o, const void* dout, const float* lse, void* dq, void* dkv,
                   void* workspace, size_t ws_bytes, int B, int Lq, int Lk, int nH, int D, int dtype, void* stream);

/* the same with dropout of the attention probabilities (models/pvt.py:60, models/twins.py:88): see vtx_attention_fwd_drop;
 * problem = image * nH + head, cell = query * Lk + key, keep [B*nH][Lq][Lk] */
int vtx_srattn_fwd_drop(const void* q, const void* kv, void* o, float* lse, int B, int Lq, int Lk, int nH, int D, int dtype,
                        float drop_p, uint64_t seed, const uint8_t* keep, void* stream);
int vtx_srattn_bwd_drop(const void* q, const void* kv, const void* o, const void* dout, const float* lse, void* dq, void* dkv,
                        void* workspace, size_t ws_bytes, int B, int Lq, int Lk, int nH, int D, int dtype, float drop_p,
                        uint64_t seed, const uint8_t* keep, void* stream);

/* ---- Halo (blocked local) attention (csrc/halo.hip, csrc/attention_long.hip; reference models/halo_transformer.py:22-115): the
 * queries of a win x win block attend to the (win + 2 halo)^2 neighbourhood around it -- out-of-image positions are ZERO key / value
 * rows that take part in the softmax (F.unfold's padding, halo_transformer.py:70-76) -- plus rel_pos[pos[q][k]][head].
 *   vtx_window_gather : dst [B * nW, (win + 2 halo)^2, nc] from channels [c0, c0 + nc) of the channels-last map [B, H, W, ld]
 *                       (halo = 0: the window partition of the queries);  vtx_window_scatter: its adjoint (sums over the
 *                       neighbourhoods that hold a token, fixed order; halo = 0: the inverse partition); c0, nc, ld multiples of 8.
 *   vtx_table_bias / _bwd: bias[h][cell] = table[pos[cell]][h] for any cell count, and the dense table gradient through the CSR of pos.
 *   vtx_xattn_fwd / _bwd: softmax(q k^T / sqrt(D) + bias) v with q [B * Lq, nH * D], kv [B * Lk, 2 * nH * D] (k | v), bias [nH][Lq][Lk]
 *                       fp32 or NULL, any Lq / Lk, D = 32 | 64 (key blocks of 64, online softmax); the backward also returns
 *                       dbias = sum over the B problems of dS (fixed order). */
int vtx_window_gather(const void* map, void* dst, int B, int H, int W, int64_t ld, int c0, int nc, int win, int halo, int dtype,
                      void* stream);
int vtx_window_scatter(const void* src, void* map, int B, int H, int W, int64_t ld, int c0, int nc, int win, int halo, int dtype,
                       void* stream);
int vtx_table_bias(const float* table, const int64_t* pos, float* bias, int64_t cells, int nH, void* stream);
int vtx_table_bias_bwd(const float* full, const int* csr_order, const int* csr_offsets, float* dtable, int64_t cells, int nH, int ntab,
                       void* stream);
int vtx_xattn_fwd(const void* q, const void* kv, void* o, float* lse, const float* bias, int B, int Lq, int Lk, int nH, int D, int dtype,
                  void* stream);
size_t vtx_xattn_bwd_workspace(int B, int Lq, int nH);
int vtx_xattn_bwd(const void* q, const void* kv, const void* o, const void* dout, const float* lse, const float* bias, void* dq,
                  void* dkv, float* dbias, void* workspace, size_t ws_bytes, int B, int Lq, int Lk, int nH, int D, int dtype,
                  void* stream);

/* vtx_xattn_* with dropout of the attention probabilities (halo_transformer.py:101); arguments as vtx_attention_fwd_drop */
int vtx_xattn_fwd_drop(const void* q, const void* kv, void* o, float* lse, const float* bias, int B, int Lq, int Lk, int nH, int D,
                       int dtype, float drop_p, uint64_t seed, const uint8_t* keep, void* stream);
int vtx_xattn_bwd_drop(const void* q, const void* kv, const void* o, const void* dout, const float* lse, const float* bias, void* dq,
                       void* dkv, float* dbias, void* workspace, size_t ws_bytes, int B, int Lq, int Lk, int nH, int D, int dtype,
                       float drop_p, uint64_t seed, const uint8_t* keep, void* stream);

/* ---- Global attention for any head width (csrc/attention_hd.hip): softmax(q k^T / sqrt(D)) v with D ANY MULTIPLE OF 8 IN 8..128 -- the
 * global-attention families only (ViT / DINO, PVT, the Twins global half; reference models/vit.py:20, pvt.py:12-30, twins.py:39-93 take
 * any dim // n_head).  No bias and no mask in these three entries: window and halo attention at any head width are vtx_attn_hdw_*
 * below, the same kernels with a bias, a mask and window addressing.  D = 32 and 64 are accepted too; the models only come here where the entries above refuse (D not in {32, 64}, or
 * vtx_attention_* at D = 32 with 160 < L <= 224).
 *   q [B * Lq, nH * D] with row stride ldq, k and v [B * Lk, nH * D] with row stride ldkv (elements): three pointers, so the packed
 *   QKV projection (k = q + nH D, v = q + 2 nH D, Lq = Lk, ldq = ldkv = 3 nH D) and the q | kv pair of the sub-sampled attention
 *   (ldq = nH D, v = k + nH D, ldkv = 2 nH D) are both served;  o, dout [B * Lq, nH * D] contiguous;  lse [B * nH * Lq] fp32;
 *   dq (row stride lddq), dk, dv (row stride lddkv): every element of the nH * D gradient columns is written.
 *   drop_p == 0: no dropout (keep must be NULL);  0 < drop_p < 1: dropout of the probabilities as vtx_attention_fwd_drop, problem =
 *   image * nH + head, cell = query * Lk + key -- vtx_attn_keep_mask exports the decisions; keep != NULL: an explicit mask of
 *   keep_cells = B * nH * Lq * Lk bytes.  A query row whose keys are all dropped stores exact zeros in o and dq.
 * Kernels templated on the padded width 32 | 64 | 96 | 128; pad columns are zero operands that are never loaded and never stored.
 * Refused before any launch: NULL pointers (VTX_ERR_NULL); D % 8 != 0, D < 8, D > 128, non-positive sizes, B * Lq or B * Lk >= 2^31,
 * a stride below nH * D, keep_cells != B * nH * Lq * Lk, drop_p outside [0, 1) (VTX_ERR_SHAPE); dtypes other than bf16 / fp32
 * (VTX_ERR_DTYPE); strides that are no multiple of 8 or bases off 16 bytes (VTX_ERR_ALIGN); ws_bytes below
 * vtx_attn_hd_bwd_workspace (VTX_ERR_WORKSPACE). */
int vtx_attn_hd_fwd(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldkv, void* o, float* lse, int B, int Lq, int Lk,
                    int nH, int D, int dtype, float drop_p, uint64_t seed, const uint8_t* keep, int64_t keep_cells, void* stream);
size_t vtx_attn_hd_bwd_workspace(int B, int Lq, int nH);
int vtx_attn_hd_bwd(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldkv, const void* o, const void* dout,
                    const float* lse, void* dq, void* dk, void* dv, int64_t lddq, int64_t lddkv, void* workspace, size_t ws_bytes, int B,
                    int Lq, int Lk, int nH, int D, int dtype, float drop_p, uint64_t seed, const uint8_t* keep, int64_t keep_cells,
                    void* stream);

/* ---- Window and halo attention for any head width and any window (csrc/attention_hd.hip, the WX instantiations): the kernels of
 * vtx_attn_hd_* with an additive score bias, a byte mask and window addressing -- Swin, the Twins locally-grouped half and Halo at
 * every D that is a multiple of 8 in 8..128 and every window size (blocks of 64 keys: no token limit).  The reference's modules take any
 * dim_head (swin_transformer.py:25-40, twins.py:109-157, halo_transformer.py:23-30; HaloNet's usual width is 16).
 *   q, k, v, ldq, ldkv, o, dout, dq, dk, dv, lddq, lddkv, drop_p, seed, keep, keep_cells: as vtx_attn_hd_*.
 *   win > 0: B counts IMAGES; token t of window n of image b is a row of the (H, W) NHWC map, shift != 0 selects the rolled partition (the
 *            roll by -win/2 and back folded into the address: what vtx_attention_fwd does with swin != 0).  q / k / v are read and o,
 *            dq, dk, dv written in map order; no partition pass.  Lq == Lk == win * win; problems = B * nW, nW = (H / win) (W / win).
 *   win == 0: B problems of plain rows b * L + t (the gathered q | kv pair of halo attention); H, W, shift are ignored.
 *   bias  fp32 [nH][Lq][Lk] or NULL: added to scale * q.k in fp32 before the online softmax, and again where the backward recomputes P.
 *   mask  uint8 [nW][Lq][Lk] or NULL (win > 0 only): a nonzero byte makes the score -inf; problem (b, n) reads mask[n].  A masked cell
 *         has p = 0 and dS = 0 exactly.  PRECONDITION: every query row has at least one unmasked key (true of every local_mask the
 *         reference builds: a token lies in its own region).  A key block that is fully masked for a query is fine.
 *   lse   [problems * nH * Lq] in the order (problem, head, query).  Dropout problem index = (image * nW + window) * nH + head, as
 *         vtx_attention_fwd_drop; keep_cells = problems * nH * Lq * Lk.
 *   dbias fp32 [nH][Lq][Lk] = the sum of dS over all problems, given exactly when bias is: the problems are cut into slabs, each slab
 *         summed in problem order into the workspace and the slabs added in slab order (deterministic, no atomics).  The table
 *         gradient follows with vtx_table_bias_bwd.
 * Refusals, before any launch: those of vtx_attn_hd_* with the same codes, and VTX_ERR_SHAPE for win < 0, H or W no multiple of win,
 * Lq != win * win or Lk != Lq with win > 0, a mask with win == 0, bias without dbias or dbias without bias in the backward;
 * VTX_ERR_WORKSPACE for ws_bytes below vtx_attn_hdw_bwd_workspace(.., has_bias). */
int vtx_attn_hdw_fwd(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldkv, void* o, float* lse, const float* bias,
                     const uint8_t* mask, int B, int Lq, int Lk, int nH, int D, int H, int W, int win, int shift, int dtype, float drop_p,
                     uint64_t seed, const uint8_t* keep, int64_t keep_cells, void* stream);
size_t vtx_attn_hdw_bwd_workspace(int B, int Lq, int Lk, int nH, int H, int W, int win, int has_bias);
int vtx_attn_hdw_bwd(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldkv, const void* o, const void* dout,
                     const float* lse, const float* bias, const uint8_t* mask, void* dq, void* dk, void* dv, int64_t lddq, int64_t lddkv,
                     float* dbias, void* workspace, size_t ws_bytes, int B, int Lq, int Lk, int nH, int D, int H, int W, int win, int shift,
                     int dtype, float drop_p, uint64_t seed, const uint8_t* keep, int64_t keep_cells, void* stream);

/* ---- Positional-encoding generator of Twins-SVT (csrc/twins_misc.hip; reference models/twins.py:25-37):
 * y = x + DepthwiseConv3x3(x) on channels-last features x, y [B, H, W, C] (C % 8 == 0, C <= 1024), w = the
 * Conv2d(C, C, 3, padding=1, bias=False, groups=C) weight [C, 1, 3, 3] fp32.  The reference permutes to NCHW, convolves and
 * permutes back (twins.py:32-35); here the taps are read in place.  adjoint != 0 mirrors the taps: vtx_dwconv3_fwd(dy, w, dx,
 * ..., 1, ...) is the input gradient.  _wgrad writes dw [C, 1, 3, 3] fp32 = sum over pixels of dy * shifted x (deterministic:
 * fixed-order partial sums in the workspace). */
int vtx_dwconv3_fwd(const void* x, const float* w, void* y, int B, int H, int W, int C, int adjoint, int dtype, void* stream);
size_t vtx_dwconv3_wgrad_workspace(int B, int H, int W, int C);
int vtx_dwconv3_wgrad(const void* x, const void* dy, float* dw, void* workspace, size_t ws_bytes, int B, int H, int W, int C,
                      int dtype, void* stream);

/* ---- Operand of the sub-sampling convolution of Twins-SVT's global attention (csrc/twins_misc.hip; reference
 * models/twins.py:69-71).  The reference reshapes its 4-D input as ``input.transpose(1, 2).reshape(B, C, H, W)``: the "image"
 * the Conv2d(C, C, r, stride r) sees is a fixed permutation of the feature map's elements (flat index f = c' H W + y W + x of
 * the (W, H, C)-ordered map), kept here as written.  x [B, H, W, C] -> out [B*(H/r)*(W/r), C*r*r], columns (c', py, px) --
 * the Conv2d weight's own memory layout [out][c'][py][px], so weight.view(out, C*r*r) is the GEMM operand and the weight
 * gradient comes out in the parameter's layout; out_t (nullable): a second, transposed copy [C*r*r, B*(H/r)*(W/r)] -- with the
 * transposed weight copy it turns the few-row / long-K convolution of the late stages (128 rows x K = 25 088) into a vtx_wgrad
 * call, i.e. a split-K launch that fills the chip; _bwd is the inverse scatter (accumulate != 0 adds into dx). */
int vtx_twins_subsample_fwd(const void* x, void* out, void* out_t, int B, int H, int W, int C, int r, int dtype, void* stream);
/* out [rows, C] (dtype) = x [rows, C] fp32 + bias [C] fp32 (nullable): fp32 split-K sums -> the compute dtype. */
int vtx_bias_cast(const float* x, const float* bias, void* out, int64_t rows, int C, int dtype, void* stream);
int vtx_twins_subsample_bwd(const void* dout, void* dx, int B, int H, int W, int C, int r, int accumulate, int dtype,
                            void* stream);

/* ---- Non-overlapping patch gather on token-major (NHWC) features: the im2col of Conv2d(C, C', p, stride = p)
 * (PVT patch embeddings of stages 2-4 and the spatial-reduction conv, pvt.py:26-29, 44-46, 112, 129-131).
 *   x [B, skip + H*W, C] (the first `skip` tokens of every image -- PVT's cls token -- are not part of the grid);
 *   out [B*(H/p)*(W/p), p*p*C] with column order (py, px, c); the conv weight is permuted to match by the host.
 * _bwd is the inverse scatter (a permutation); accumulate != 0 adds into dx (the gradient that also arrives
 * through the query path), rows of skipped tokens are left untouched. */
int vtx_patchify_fwd(const void* x, void* out, int B, int H, int W, int C, int p, int skip, int dtype, void* stream);
int vtx_patchify_bwd(const void* dout, void* dx, int B, int H, int W, int C, int p, int skip, int accumulate, int dtype,
                     void* stream);

/* ---- Position-embedding add with optional cls token (PVT PatchEmbedding, pvt.py:133-137):
 *   out[b, 0] = cls + pos[0] (has_cls), out[b, s + t] = x[b, t] + pos[s + t], s = has_cls.
 *   x [B, T, C] of dtype, cls [C] / pos [s + T, C] fp32; _bwd: dx = dout[:, s:], dcls = sum_b dout[b, 0],
 *   dpos = sum_b dout[b] (fp32, deterministic). */
int vtx_add_pos_fwd(const void* x, const float* cls, const float* pos, void* out, int B, int T, int C, int dtype,
                    void* stream);
int vtx_add_pos_bwd(const void* dout, void* dx, float* dcls, float* dpos, int B, int T, int C, int dtype, void* stream);

/* ---- Row-wise L2 normalisation y = x / max(||x||_2, eps) (F.normalize of the DINO head, models/vit.py:258) and its
 * backward dx = (dy - y sum(y o dy)) / ||x|| where ||x|| >= eps, dx = dy / eps where the clamp is active (its derivative is
 * zero: F.normalize under autograd); nrm [rows] fp32 = the UNCLAMPED ||x||, saved by the forward; eps: the forward's. */
int vtx_l2norm_fwd(const void* x, void* y, float* nrm, int64_t rows, int C, float eps, int dtype, void* stream);
int vtx_l2norm_bwd(const void* dy, const void* y, const float* nrm, void* dx, int64_t rows, int C, float eps, int dtype,
                   void* stream);

/* ---- Device-side input pipeline (csrc/input.hip): per-sample mixup / cutmix
 * (reference mix_dataset.py:36-90) + Normalize + RandomErasing in its three colour modes (reference transforms.py:309-418;
 * factory.py:177-181 configures mode "pixel") of a device-resident batch in one pass.  The random plan is drawn on the
 * host in the reference's order (vtx.input_pipeline.plan_batch): device array of N records
 *   {int partner, mode (0 none | 1 mixup | 2 cutmix); float ratio; int x1, y1, x2, y2, nrect, top[4], left[4];
 *    short eh[4], ew[4]; int fmode (0 const | 1 rand | 2 pixel), foff[4]}
 *   (vtx_mix_plan_bytes() = 100 bytes each; at most vtx_mix_max_rects() rectangles);
 * fills: fp32 table of the host-drawn normal values (Tensor.normal_ with the reference's shapes), rectangle r of a sample
 *   reads [C] (rand) or [C][eh][ew] (pixel) floats at foff[r]; may be NULL when every fmode is 0.
 * x [N, C, H, W] uint8 (in_u8: scaled by 1/255 like ToTensor) or fp32, W % 4 == 0;
 * out: [N, C, H, W] fp32 (out_nhwc_bf16 == 0: the reference's model input) or [N, H, W, C] bf16 (C in {1, 3, 4}) -- the
 *   layout vtx_patch_gather_nhwc consumes, so the patch-embedding input is written once, in place of train.py:267's
 *   fp32 NCHW batch + the permute / patchify copies of swin_transformer.py:371, 15-22. */
size_t vtx_mix_plan_bytes(void);
int vtx_mix_max_rects(void);
int vtx_mix_normalize_erase(const void* x, int in_u8, const void* plan, const float* mean, const float* stdv,
                            const float* fills, void* out, int out_nhwc_bf16, int N, int C, int H, int W, void* stream);

/* ---- RandAugment on the device (csrc/randaug.hip): the PIL-image mix of reference
 * mix_dataset.py:63-86 (Image.blend / paste) followed by the RandAugment ops of reference autoaugment.py:586-678, per
 * image, bit-exact to PIL, for the default mix_before_aug order (factory.py:184-187).  All random draws are made on the
 * host (vtx.input_pipeline.RandAugmentPlan); plan = device array of N records
 *   {int partner, mode (0 none | 1 mixup | 2 cutmix); float alpha (Image.blend's, = 1 - ratio); int x1, y1, x2, y2
 *    (box: columns [x1, x2), rows [y1, y2)); int nops; int fill[4]; {int code; int p[6]; float f;} op[8]}
 *   (vtx_randaug_plan_bytes() = 304 bytes each; at most vtx_randaug_max_ops() ops; op codes and parameters in
 *   csrc/randaug.hip).
 * x, scratch, out: [N, 3, H, W] uint8 (RGB planes), pairwise distinct; out is what vtx_mix_normalize_erase then reads
 * with mix mode 0 (ToTensor / Normalize / RandomErasing). */
size_t vtx_randaug_plan_bytes(void);
int vtx_randaug_max_ops(void);
int vtx_randaug_apply(const void* x, const void* plan, void* scratch, void* out, int N, int C, int H, int W, void* stream);

/* ---- Crop + BICUBIC resize + flip on the device (csrc/resample.hip): RandomResizedCrop(size,
 * BICUBIC) + RandomHorizontalFlip of reference factory.py:170-171 (and the crops of DINOAugment, transforms.py:249-279) and
 * Resize + CenterCrop of factory.py:215-222, bit-exact to PIL's 8-bit resample of the CROPPED image (img.crop(box).resize(
 * size, BICUBIC): filter windows clamp at the crop's edges).  All random draws are made on the host
 * (vtx.input_pipeline.RandomResizedCropPlan); table = device array of M records, one per OUTPUT image (several may name one
 * source):
 *   {int64 src_off (byte offset of the source's row 0 in buf); int src_h, src_w, stride (bytes per source row);
 *    int top, left, ch, cw (crop rectangle); int res_h, res_w (size the crop is resampled to);
 *    int win_top, win_left (out = rows [win_top, win_top + S_h) x columns [win_left, win_left + S_w) of the resampled image:
 *    0, 0 and res = S for a plain resized crop; the CenterCrop offsets for Resize + CenterCrop); int flip; int pad}
 *   (vtx_resample_plan_bytes() = 64 bytes each).
 * buf: buf_bytes device bytes, the sources in PIL's layout (H x W x 3 uint8, RGB interleaved); ws: device workspace of
 * vtx_resample_workspace_bytes(M, S_h, S_w) bytes (the coefficient tables, built on the device); out: [M, 3, S_h, S_w]
 * uint8 -- what vtx_randaug_apply and vtx_mix_normalize_erase take.  Supported: crop side / output side <= 16 on both axes
 * (at most vtx_resample_max_taps() = 65 filter taps), up-scaling included, 3 * S_w <= ~2500.  A record outside that range,
 * outside its source or outside buf is the caller's error: its image is zero-filled, nothing of it is read.
 * vtx_resample_coeffs: the tables of one axis (length L resampled to S, outputs [first, first + n)) as the kernel builds them:
 *   table = (2 + max_taps) * n device int32:  xmin[n] | count[n] | coef[max_taps][n]  (22-bit fixed point, unused taps 0). */
size_t vtx_resample_plan_bytes(void);
int vtx_resample_max_taps(void);
size_t vtx_resample_workspace_bytes(int M, int S_h, int S_w);
int vtx_resample_coeffs(int L, int S, int first, int n, void* table, void* stream);
int vtx_resized_crop(const void* buf, size_t buf_bytes, const void* table, void* ws, size_t ws_bytes, void* out, int M, int S_h,
                     int S_w, void* stream);

/* Down-scales beyond 16, opt-in (vtx.input_pipeline: max_downscale): a second launch over the records of the SAME table that
 * vtx_resized_crop zero-filled because a side has more than 65 taps.  idx = device int32[L], the indices of those records; only
 * their images of out ([M, 3, S_h, S_w], the tensor vtx_resized_crop wrote) are written, everything else is left untouched.
 * max_taps: the size of the coefficient tables, 1..513 (513 = crop side / output side 128; a chosen bound) and at least the
 * largest tap count among the L records; ws = vtx_resample_long_workspace_bytes(L, S_h, S_w, max_taps) device bytes
 * = L * (2 + max_taps) * (S_h + S_w) int32 (0 for arguments the entry refuses).  Same arithmetic, bit-exact to PIL: a vertical
 * window longer than the LDS tile is summed over several tile loads, the int32 accumulators staying in registers.  Argument
 * violations are VTX_ERR_SHAPE before any launch; a record with more than max_taps taps, outside its source or outside buf is
 * zero-filled as by vtx_resized_crop; an index outside [0, M) is skipped. */
size_t vtx_resample_long_workspace_bytes(int L, int S_h, int S_w, int max_taps);
int vtx_resized_crop_long(const void* buf, size_t buf_bytes, const void* table, const void* idx, int L, int max_taps, void* ws,
                          size_t ws_bytes, void* out, int M, int S_h, int S_w, void* stream);

/* ---- Baseline JPEG decode, the first stage of the input pipeline (csrc/jpeg_host.h + csrc/jpeg.hip; SURVEY section 8 row F4;
 * reference dataset.py:144, Image.open(buffer).convert("RGB")): bit-exact to PIL's decoder, i.e. libjpeg's default integer path
 * (JDCT_ISLOW, fancy upsampling, table-driven YCbCr -> RGB).  The Huffman bit stream is decoded on the HOST into de-zigzagged
 * int16 coefficient blocks (reentrant, no global state: one call per image from any thread) -- or, with the entries of the next
 * section, on the device into the same bytes; dequantisation, inverse DCT,
 * chroma upsampling and colour conversion run on the device, two launches per batch; the pixels land as H x W x 3 uint8 rows in
 * the byte buffer vtx_resized_crop reads.
 * Accepted: SOF0 (or SOF1 with 8-bit tables), 8-bit, one interleaved scan, 1 component or YCbCr with luma sampling (1,1), (2,1)
 * or (2,2) and chroma 1x1, restart intervals; progressive (SOF2) and multi-scan sequential files only through the opt-in entries
 * below (vtx_jpeg_info_ex / vtx_jpeg_entropy_decode_ms, reasons 16 and 17).  Refused with VTX_ERR_JPEG and a reason (VTX_JPEG_* of
 * csrc/jpeg_host.h):
 * 1 not a JPEG / malformed header, 2 progressive, 3 arithmetic, 4 lossless / hierarchical, 5 12-bit samples or 16-bit tables,
 * 6 components other than 1 or 3, 7 other sampling factors, 8 more than one scan, 9 an Adobe transform other than YCbCr,
 * 10 component ids R, G, B without JFIF, 11 DNL, 12 zero dimensions, 13 corrupt or truncated entropy-coded data, 14 a window
 * outside the image or a coefficient range outside the caller's buffer, 15 more than 2^26 blocks or 2^28 pixels to store (the
 * size functions return 0 for such an image or window, and for a VtxJpegInfo that no accepted header produces).
 *   VtxJpegInfo: {int width, height, ncomp, hs, vs (luma sampling), mcux, mcuy, reason, restart, reserved[3]}
 *   window = {row0, col0, rows, cols} in pixels, NULL = the whole image: only the MCUs the window touches, plus the one-sample
 *     chroma context of the upsampling, are stored (the bit stream is still walked in full) and the device writes exactly
 *     the window -- bit-equal to the full decode cropped.
 *   plan record (vtx_jpeg_plan_bytes() = 480 bytes, csrc/jpeg_host.h VtxJpegPlan): geometry and sampling, the stored MCU
 *     rectangle, the window, the byte offsets offs[3] = {coefficients, component planes, output pixels} given to
 *     vtx_jpeg_entropy_decode, and the dequantisation table of each component (3 x 64 uint16, natural order).
 * vtx_jpeg_entropy_decode: coef / coef_bytes = the caller's (pinned) coefficient memory; the image's blocks go to coef + offs[0]
 *   (vtx_jpeg_coef_bytes(info, window) bytes: luma blocks row-major, then Cb, then Cr, 64 int16 each).  *reason may be NULL.
 * vtx_jpeg_decode: coef = the DEVICE copy of that memory; plans = n records in HOST memory -- every record is checked against
 *   coef_bytes, ws_bytes and out_bytes before anything is launched (VTX_ERR_JPEG for a record that would reach outside), then
 *   copied to the head of ws on `stream` (pinned memory must stay unchanged until the stream has passed that copy); ws =
 *   vtx_jpeg_workspace_bytes(n, P) device bytes, 8-byte aligned, P = the end of the records' plane ranges (each
 *   vtx_jpeg_plane_bytes(info, window) bytes at offs[1], a multiple of 8); out: device bytes, image i's window as rows x cols x 3
 *   uint8 at its offs[2]. */
int vtx_jpeg_info(const void* data, size_t len, void* info);
size_t vtx_jpeg_plan_bytes(void);
size_t vtx_jpeg_coef_bytes(const void* info, const int* window);
size_t vtx_jpeg_plane_bytes(const void* info, const int* window);
size_t vtx_jpeg_workspace_bytes(int n, size_t plane_bytes);
int vtx_jpeg_entropy_decode(const void* data, size_t len, const int* window, void* coef, size_t coef_bytes, const long long* offs,
                            void* plan, int* reason);
int vtx_jpeg_decode(const void* coef, size_t coef_bytes, const void* plans, int n, void* ws, size_t ws_bytes, void* out,
                    size_t out_bytes, void* stream);

/* Multi-scan JPEG, opt-in (csrc/jpeg_multiscan.h; vtx.input_pipeline: jpeg_scans="any"): progressive DCT (SOF2) and sequential
 * files whose scans do not each hold every component, through the HOST stage into the same coefficient blocks and plan record,
 * so that vtx_jpeg_decode and the device kernels run unchanged.  Every scan up to EOI is walked (DHT / DQT / DRI between scans;
 * DC and AC, first and refinement scans, interleaved or not, EOB runs and correction bits; restart intervals counted in the
 * scan's own MCUs).  A refinement needs every block's earlier state: the decode works on the whole image's coefficients in a
 * caller-owned scratch (zeroed by the call) and copies the window's MCU rectangle out; the library allocates nothing.
 *   vtx_jpeg_info_ex: flags 0 = vtx_jpeg_info; bit 0 accepts those files and records the kind in info.reserved[0]: 0 single scan,
 *     1 multi-scan sequential, 2 progressive.  Components, sampling, precision, Adobe and RGB-id rules are vtx_jpeg_info's.
 *   vtx_jpeg_scratch_bytes(info): 0 for kind 0; all blocks of the padded MCU grid x 128 bytes otherwise; 0 for more than 2^22
 *     blocks (512 MiB), which vtx_jpeg_entropy_decode_ms refuses with reason 15.
 *   vtx_jpeg_entropy_decode_ms: vtx_jpeg_entropy_decode's arguments plus the scratch (2-byte aligned; NULL for a kind-0 file, which
 *     goes through vtx_jpeg_entropy_decode); a scratch too small is reason 14.
 * Further reasons: 16 an invalid scan script -- Ss > Se, Se > 63, a DC scan with Se != 0, an AC scan of several components,
 *   Al > 13, Ah that is neither 0 for a coefficient not yet sent nor the Al of that coefficient's previous scan, AC before the
 *   component's first DC scan, a sequential scan other than Ss = 0, Se = 63, Ah = Al = 0 or a component in two of them, more than
 *   256 scans (libjpeg's JERR_BAD_PROGRESSION / JERR_BAD_PROG_SCRIPT, and its JWRN_BOGUS_PROGRESSION warning is a refusal here);
 *   17 an incomplete progression: at EOI coefficients 0..9 of every component must have ended at Al = 0 (libjpeg smooths blocks
 *   otherwise, differently in different versions), and every component of a sequential file must have had its scan.
 *   Coefficients above 9 never sent are zero, those left at Al > 0 keep their partial value, as in libjpeg.  Data that ends before
 *   EOI or inside a scan is reason 13. */
int vtx_jpeg_info_ex(const void* data, size_t len, void* info, int flags);
size_t vtx_jpeg_scratch_bytes(const void* info);
int vtx_jpeg_entropy_decode_ms(const void* data, size_t len, const int* window, void* coef, size_t coef_bytes, const long long* offs,
                               void* plan, void* scratch, size_t scratch_bytes, int* reason);

/* ---- The entropy (Huffman) stage on the device (csrc/jpeg_sync.h + csrc/jpeg_entropy.hip; DESIGN.md "Entropy stage on the
 * device"): an alternative to vtx_jpeg_entropy_decode that leaves only the header parse and a byte scan on the host.  The
 * coefficient buffer is device memory: it has the same bytes vtx_jpeg_entropy_decode writes and vtx_jpeg_decode reads it as before.
 *   scan record (vtx_jpeg_scan_bytes() = 8640 bytes, csrc/jpeg_sync.h JsScan): geometry, the stored rectangle, the restart
 *     interval, offsets, and the DC / AC Huffman table of each component.
 *   segment table: 16 bytes per restart interval (one for a file without markers): where the interval's bytes lie and how many
 *     blocks it holds.  stream: the entropy-coded bytes with the stuffed zero bytes and the markers removed.
 * vtx_jpeg_scan_prepare (host, reentrant): offs = {coefficient, plane, output, stream, segment table} byte offsets and the index
 *   of the image's first subsequence; writes the plan record of vtx_jpeg_entropy_decode, the scan record, the segment table at
 *   segs + offs[4] and the bytes at stream + offs[3].  Same reason codes as vtx_jpeg_entropy_decode for every header refusal and
 *   for a restart marker that is missing or out of sequence (13); 15 also for a scan of 2^28 bytes or more.  Bad codes and
 *   truncated data are found by the decode.
 * vtx_jpeg_scan_stream_bytes / _segment_bytes / _subsequences: upper bounds of what prepare writes for one file (0 for what it
 *   refuses); vtx_jpeg_entropy_workspace_bytes(n, segment bytes, subsequences): the workspace of a batch, 16-byte aligned.
 * vtx_jpeg_entropy_launch: stream_dev = the DEVICE copy of the bytes; segs / scans = HOST tables, every record and segment
 *   checked against stream_bytes, seg_bytes, coef_bytes and ws_bytes before anything is launched (VTX_ERR_JPEG), then copied to
 *   the head of ws on `stream`; coef / status: device.  One launch, one workgroup per image, no synchronisation, no allocation.
 *   status[i] = 0, 13 (corrupt or truncated entropy-coded data: exactly where vtx_jpeg_entropy_decode says 13) or 100 (not
 *   converged within `cap` rounds, cap <= 0 meaning vtx_jpeg_round_cap(): decode that file with vtx_jpeg_entropy_decode).  Every block of an image's
 *   coefficient range is written whatever the status; nothing outside it is.
 * vtx_jpeg_entropy_emulate: the same arguments in HOST memory, the kernel's algorithm with its lanes as a sequential loop;
 *   rounds[i] (may be NULL) = rounds run; cap <= 0: vtx_jpeg_round_cap(). */
size_t vtx_jpeg_scan_bytes(void);
size_t vtx_jpeg_scan_stream_bytes(const void* data, size_t len);
size_t vtx_jpeg_scan_segment_bytes(const void* info);
size_t vtx_jpeg_scan_subsequences(const void* info, size_t stream_bytes);
size_t vtx_jpeg_entropy_workspace_bytes(int n, size_t seg_bytes, size_t nsub);
int vtx_jpeg_round_cap(void);
int vtx_jpeg_subsequence_bits(void);
int vtx_jpeg_scan_prepare(const void* data, size_t len, const int* window, const long long* offs, void* stream, size_t stream_cap,
                          void* segs, size_t seg_cap, void* scan, void* plan, int* reason);
int vtx_jpeg_entropy_launch(const void* stream_dev, size_t stream_bytes, const void* segs, size_t seg_bytes, const void* scans, int n,
                            void* coef, size_t coef_bytes, void* ws, size_t ws_bytes, int* status, int cap, void* stream);
int vtx_jpeg_entropy_emulate(const void* stream_host, size_t stream_bytes, const void* segs, size_t seg_bytes, const void* scans, int n,
                             void* coef, size_t coef_bytes, void* ws, size_t ws_bytes, int* status, int* rounds, int cap);

/* ---- DINOAugment after the crop, on the device (csrc/dinoaug.hip; reference
 * transforms.py:225-294): RandomApply(ColorJitter) -> RandomGrayscale -> GaussianBlur -> Solarize per crop, one launch,
 * bit-exact to the PIL operations behind them (ImageEnhance, convert("HSV") / convert("RGB"), convert("L"),
 * ImageFilter.GaussianBlur, ImageOps.solarize).  All random draws are made on the host
 * (vtx.input_pipeline.DinoAugmentPlan); plan = device array of M records
 *   {int nops (0..4 jitter ops, applied in order); int code[4] (1 brightness | 2 contrast | 3 saturation | 4 hue);
 *    float f[4] (the enhance factor of codes 1..3, >= 0); int shift[4] (code 4: the integer added to the H plane, modulo 256);
 *    int gray (convert("L") x 3); int blur_r, blur_ww, blur_fw (ImagingBoxBlur's integer radius and 24-bit weights of one
 *    box pass, computed on the host from the Gaussian radius with PIL's float steps; blur_ww == 0: no blur);
 *    int solarize (threshold 0..256, -1: none)}
 *   (vtx_dinoaug_plan_bytes() = 72 bytes each; blur_r <= vtx_dinoaug_max_box_radius() = 7).
 * x: [M, 3, H, W] uint8 (what vtx_resized_crop writes); out: [M, 3, H, W] uint8, distinct from x (what
 * vtx_mix_normalize_erase then reads); scratch: vtx_dinoaug_scratch_bytes(M, H, W) device bytes -- 0 (scratch may be NULL)
 * while the blur's two planes fit in LDS (2 * H * W <= 144 KB: every crop up to 271 x 271), the batch's size beyond. */
size_t vtx_dinoaug_plan_bytes(void);
int vtx_dinoaug_max_box_radius(void);
size_t vtx_dinoaug_scratch_bytes(int M, int H, int W);
int vtx_dinoaug_apply(const void* x, const void* plan, void* scratch, void* out, int M, int C, int H, int W, void* stream);

/* ---- Fused optimizer tail (csrc/optim.hip): nn.utils.clip_grad_norm_ + torch.optim.AdamW.step of the reference's
 * train step (train.py:285-299) as two multi-tensor passes.  Tensors are given as HOST arrays of n device pointers
 * (fp32, any 4-byte alignment) and element counts; the addresses travel in kernel arguments (64 tensors per launch).
 *   vtx_grad_sqnorm: norm_out[0] = sum over all tensors of g^2, norm_out[1] = its square root (deterministic: fixed
 *                    summation order, no atomics); partial = sum_i ceil(numel_i / vtx_opt_chunk()) floats of workspace.
 *   vtx_adamw_step:  step t >= 1 of AdamW (decoupled decay first, bias-corrected, eps added to sqrt(v)/sqrt(1-b2^t)),
 *                    per-tensor lr / weight decay, on g * min(1, max_norm / (norm[1] + 1e-6)) when max_norm > 0
 *                    (norm = vtx_grad_sqnorm's device output); gradients are not modified. */
int vtx_opt_chunk(void);
int vtx_grad_sqnorm(int n, const float* const* g, const int64_t* numel, float* partial, float* norm_out, void* stream);
int vtx_adamw_step(int n, float* const* p, const float* const* g, float* const* m, float* const* v,
                   const int64_t* numel, const float* lr, const float* wd, const float* norm, float max_norm,
                   float beta1, float beta2, float eps, int t, void* stream);

/* Momentum (EMA) update of the DINO teacher / an EMA model: p_i = m * p_i + (1 - m) * g_i for n fp32 tensors given as
 * HOST arrays of device pointers (train_dino.py:258-263, train_util.py:70-76). */
int vtx_ema_update(int n, float* const* p, const float* const* g, const int64_t* numel, float m, void* stream);

/* Model EMA (reference train_util.py:70-84 ``accumulate``, called from train.py:304-316), both weights from the caller:
 *     e_i = fma(p_i, alpha, e_i * decay)        (one rounded product, then one fused multiply-add: mul_ then add_(alpha=))
 * alpha is the CALLER's: the reference forms 1 - decay in double and rounds once (9.99999975e-06 for decay 0.99999, where the
 * fp32 difference 1.f - decay of vtx_ema_update is 1.00135803e-05).  decay = 0 copies alpha * p (p itself for alpha = 1),
 * decay = 1 with alpha = 0 leaves e unchanged: both exact for finite values.
 *   vtx_ema_update2:    n pairs (e, p) as HOST arrays of device pointers (fp32, any 4-byte alignment), one pass.
 *   vtx_adamw_ema_step: vtx_adamw_step with the EMA of the NEW parameter written in the same pass; ema = HOST array of n
 *                       device pointers, a NULL entry = that tensor has no target.  p, m, v are bit-identical to
 *                       vtx_adamw_step's, every target bit-identical to vtx_ema_update2 of the updated parameter.
 *   vtx_opt_ema_pack:   tensors per launch of these two entries (their kernel arguments carry one address more per tensor). */
int vtx_opt_ema_pack(void);
int vtx_ema_update2(int n, float* const* e, const float* const* p, const int64_t* numel, float decay, float alpha,
                    void* stream);
int vtx_adamw_ema_step(int n, float* const* p, const float* const* g, float* const* m, float* const* v,
                       const int64_t* numel, const float* lr, const float* wd, const float* norm, float max_norm,
                       float beta1, float beta2, float eps, int t, void* stream, float* const* ema, float decay,
                       float alpha);

/* ---- DINO loss (csrc/dino.hip; reference loss.py:122-152): forward value and gradient w.r.t. the student logits in
 * one sweep, plus the teacher column sums of update_center.
 *   student [n_crop*B, K], teacher [2*B, K] (dtype), center [K] fp32 (read only); K % 8 == 0;
 *   loss_rows [n_crop*B] fp32 with loss = sum(loss_rows) / ((2 n_crop - 2) B);
 *   dstudent [n_crop*B, K] (dtype) = gscale * d loss / d student;  batch_center [K] fp32 = sum of the teacher rows;
 *   workspace: vtx_dino_loss_workspace(B, K) bytes. */
size_t vtx_dino_loss_workspace(int B, int K);
int vtx_dino_loss(const void* student, const void* teacher, const float* center, void* workspace, size_t ws_bytes,
                  float* loss_rows, void* dstudent, float* batch_center, int n_crop, int B, int K, float student_temp,
                  float teacher_temp, float gscale, int dtype, void* stream);

/* ---- MixLoss of the supervised train step (csrc/dino.hip; reference loss.py:53-86, train.py:274-276): label-smoothed KL
 * between log_softmax(logits) and r * smooth(label1) + (1 - r) * smooth(label2), reduction "mean"; value and gradient
 * in one sweep.  logits / dlogits [B, K] (dtype), labels [B] int64, ratio [B] fp32; loss = sum(loss_rows) / B. */
int vtx_mix_loss(const void* logits, const int64_t* label1, const int64_t* label2, const float* ratio, void* dlogits,
                 float* loss_rows, int B, int K, float eps, float gscale, int dtype, void* stream);

/* ---- Loss and prec@k meters (csrc/metrics.hip; reference train.py:277-281, 335-386, train_util.py:34-67): per-row
 * cross entropy and the label's rank in one sweep of the (B, K) logits, then -- in the same call, on the same stream --
 * the batch added to a device meter.  No host synchronisation; the caller reads the meter when it wants the numbers.
 *   logits [B, K] (dtype; any row alignment, any K >= 1), labels [B] int64;
 *   ce_rows [B] fp32 = logsumexp(row) - row[label]  (F.cross_entropy, reduction "none");
 *   rank [B] int32   = #{j : x_j > x_l} + #{j < l : x_j == x_l}: the label's position in a STABLE descending sort --
 *                      among equal logits the lower class index ranks first.  The label is in the top k exactly when
 *                      rank < k.  (torch.topk leaves the order of ties unspecified; this rule is the contract.)
 *   meter [2 + nk] fp64 or NULL (rows only): [n, loss_sum, hits_ks0, hits_ks1, ...]; the call ADDS the batch's counted
 *                      rows, their cross-entropy sum and their rows with rank < ks[i].  One workgroup, fixed summation
 *                      order, no atomics: the same inputs give the same bits.  ks: HOST array of nk (0..8) values >= 1,
 *                      passed to the kernel by value.
 *   loss_override     NULL, or one fp32 DEVICE scalar (a batch-mean loss): loss_sum += *loss_override * loss_scale *
 *                      (counted rows) replaces the cross-entropy sum -- how the training loop meters MixLoss
 *                      (losses.update(loss.item() * grad_accum, batch), train.py:279).
 * Edge rules:
 *   - NaN logits order above +inf (as torch.topk does) and tie with each other by class index; the cross entropy of a
 *     row that holds one is NaN.
 *   - -inf logits (masked classes) are allowed when the row has at least one finite logit: they add nothing to the
 *     sum of exponentials.
 *   - label == ignore_index (nn.CrossEntropyLoss's default is -100): ce_rows = 0, rank = -1, the row is NOT counted.
 *   - any other label outside [0, K) is never used as an index: ce_rows = NaN, rank = K, the row IS counted -- the
 *     poison shows in the epoch's loss.
 *   - ks[i] > K: every counted row is a hit (rank <= K < ks[i]).
 * Errors: VTX_ERR_NULL (logits / labels / ce_rows / rank, or ks with nk > 0), VTX_ERR_SHAPE (B, K < 1; nk outside 0..8;
 * ks[i] < 1), VTX_ERR_DTYPE, VTX_ERR_ALIGN (logits not aligned to its element size). */
int vtx_cls_metrics(const void* logits, const int64_t* labels, float* ce_rows, int32_t* rank, double* meter,
                    const int32_t* ks, int nk, const float* loss_override, float loss_scale, int B, int K,
                    int64_t ignore_index, int dtype, void* stream);

/* ---- Weighted k-nearest-neighbour evaluation of frozen features (csrc/knn.hip, csrc/knn_select.h): the measure DINO
 * runs are judged by.  The search streams the bank through LDS and never writes the (M, N) score matrix; the vote turns a
 * query's neighbour list into the rank of its label.  No host synchronisation.
 *
 * vtx_knn_topk: q [M, D] queries, f [N, D] bank (both dtype, rows used as given -- nothing is normalised here),
 *   val [M, k] fp32, idx [M, k] int32.
 *   - Order.  The score of a pair is the fp32-accumulated dot product of its two rows.  Row m of the output holds the
 *     first k bank rows in the total order "higher score first, among equal scores the lower bank index first" -- a STABLE
 *     descending sort of the score row, the rule of vtx_cls_metrics -- listed in that order.  The order is total, so the
 *     answer is unique.
 *   - Pair-local scores.  The score of a pair depends on its two rows only (one MFMA chain over D for every pair): not
 *     on M, N, the tile the pair falls in or splits.  The same pair gives the same bits in every call.
 *   - splits: the bank is cut into `splits` (1..64; 0 = choose from M and N) slabs of consecutive rows; every slab
 *     writes its own k-list to the workspace and a second launch merges them under the same order.  The answer does
 *     not depend on splits.  Workspace: vtx_knn_workspace_bytes(M, N, k, splits) = 8 M splits k bytes (0 for one split),
 *     4-byte aligned; ws may be NULL when that is 0.
 *   - Non-finite scores give unspecified neighbours (a NaN score is treated as -inf); even then every returned index
 *     lies in [0, N) and the call ends.
 *   Errors, all before any launch: VTX_ERR_NULL (q, f, val, idx; ws when a workspace is needed), VTX_ERR_SHAPE (M < 1,
 *   N < 1, M or N >= 2^31, D > 1024, k < 1, k > 256, k > N, splits outside 0..64), VTX_ERR_ALIGN (D % 8 != 0; q or f not
 *   16-byte aligned), VTX_ERR_DTYPE, VTX_ERR_WORKSPACE (ws_bytes short).
 *
 * vtx_knn_vote: val / idx [M, L] (a search result, L <= 256), bank_labels [N] int64, query_labels [M] int64, ks: HOST
 *   array of nk (1..8) values in 1..L, C classes, temperature T > 0.  Per query and per k in ks:
 *     w_i      = expf(val_i / T) in fp32;
 *     votes[c] = sum of w_i over the neighbours i < k whose bank label is c, added in neighbour order in fp32 (the vote
 *                at a smaller k is a prefix of the vote at a larger one);
 *     rank     = #{c : votes[c] > votes[l]} + #{c < l : votes[c] == votes[l]} over the classes [0, C), l the query's
 *                label: its position in a STABLE descending sort of the votes.  Classes without a neighbour have vote 0
 *                and take part in the tie rule.
 *   rank [M, nk] int32; pred [M, nk] int32 = the class of rank 0.
 *   Labels are compared, never used as indices: a bank label outside [0, C) votes for no class, a query label outside
 *   [0, C) gives rank = C -- the row is counted and never a hit; an idx outside [0, N) is a neighbour of no class.
 *   meter [1 + 2 nk] fp64 or NULL: [n, top1_ks0, top5_ks0, top1_ks1, top5_ks1, ...]; the call ADDS M and the rows with
 *   rank < 1 and with rank < min(5, ks[i]).  One workgroup, fixed summation order, no atomics.
 *   Errors: VTX_ERR_NULL (any pointer but meter), VTX_ERR_SHAPE (M, N < 1 or >= 2^31; L outside 1..256; C < 1; nk outside
 *   1..8; ks[i] outside 1..L; T not > 0).
 *
 * vtx_knn_merge_lists: the search over a bank of N rows that is cut into nlist (1..64) shards of consecutive rows, one per
 *   rank: every shard was searched on its own (vtx_knn_topk with k_s = min(k, rows of the shard)) and the lists meet here.
 *   lens, bases: HOST arrays of nlist values, copied into the launch (no device copy, no synchronisation): list s holds
 *   lens[s] (0..k) real pairs in order, its indices are local to shard s, whose row 0 is row bases[s] of the bank.
 *   List s of query m starts at element m * row_stride + s * list_stride of lval / lidx; places at or beyond lens[s] are
 *   never read.  Two layouts through the one entry: rank-major, as a gather of the ranks' [rows, k] results leaves them
 *   (list_stride = rows * k, row_stride = k, the pointers advanced to the caller's first query), and query-major, as the
 *   split workspace of vtx_knn_topk (row_stride = nlist * k, list_stride = k).
 *   val [M, k] fp32, idx [M, k] int32: the first k pairs of all lists in the order "higher score first, among equal scores
 *   the lower global index first", global index = bases[s] + local index.  Scores are pair-local, so this is bit for bit
 *   the answer of vtx_knn_topk over the whole bank.  A NaN score orders as -inf; on lists that are not ordered the
 *   neighbours are unspecified, and even then every written index lies in [0, N) and the call ends.
 *   Errors, all before any launch: VTX_ERR_NULL (any pointer), VTX_ERR_SHAPE (M < 1 or >= 2^31; N < 1 or >= 2^31 - 1; nlist
 *   outside 1..64; k outside 1..256; a lens[s] outside 0..k or above the rows of shard s = bases[s + 1] - bases[s], N -
 *   bases[s] for the last; sum of lens < k; bases[0] < 0, bases decreasing, bases[nlist - 1] > N; list_stride < k with
 *   nlist > 1; row_stride < k with M > 1). */
size_t vtx_knn_workspace_bytes(int64_t M, int64_t N, int k, int splits);
int vtx_knn_topk(const void* q, const void* f, float* val, int32_t* idx, int64_t M, int64_t N, int D, int k, int splits,
                 void* ws, size_t ws_bytes, int dtype, void* stream);
int vtx_knn_vote(const float* val, const int32_t* idx, const int64_t* bank_labels, const int64_t* query_labels,
                 int32_t* rank, int32_t* pred, double* meter, const int32_t* ks, int nk, int64_t M, int L, int64_t N, int C,
                 float T, void* stream);
int vtx_knn_merge_lists(const float* lval, const int32_t* lidx, float* val, int32_t* idx, const int32_t* lens,
                        const int32_t* bases, int nlist, int64_t M, int k, int64_t row_stride, int64_t list_stride, int64_t N,
                        void* stream);

/* ---- Linear-probe evaluation of frozen features (csrc/probe.hip): H linear heads (1..32), one per (learning rate,
 * weight decay) pair, trained at once on rows of a feature bank.  The (rows, classes) logit matrix is never written.
 * No host synchronisation, no global state, no floating-point atomics: the same inputs give the same bits.
 *
 * Common layouts: x [N, D] of dtype (bf16 or fp32), rows used as given; rows: int32 [M] indices into x and labels, or NULL
 * for rows 0..M-1 (repeats are allowed; an index outside [0, N) is clamped into it, never used as given); labels [N]
 * int64; w [H, C, D] of dtype; bias [H, C] fp32 or NULL.  D is a multiple of 8 in 8..1024, C >= 1, 1 <= M <= N < 2^31.
 *
 * vtx_probe_fwd: lse, ce [H, M] fp32, pred [H, M] int32, meter [H, 3] fp64 or NULL.
 *   - Pair-local logits.  The logit of (row, class) is the fp32-accumulated dot product of the two rows -- one MFMA chain
 *     over D for every pair (v_mfma_f32_16x16x32_bf16, or the exact 16x16x4_f32 chain in fp32) -- followed by one fp32 add
 *     of the bias.  It depends on its two rows and the bias only: not on M, H, the head's index, rows or the tile the
 *     pair falls in.  The same pair gives the same bits in every call, and the backward recomputes the same bits.
 *   - lse = max + __logf(sum), from a running maximum and a rescaled running sum of __expf(logit - max) over the classes in
 *     ascending order; pad classes of the last class tile add nothing to the sum and are never a candidate.
 *   - ce = lse - logit of the label.
 *   - pred = the first class of the highest logit: among equal logits the lower class index wins -- the rule of
 *     vtx_cls_metrics, so pred == label exactly when rank < 1 there.
 *   - A label outside [0, C) is never used as an index: ce = NaN, the row is counted and never a hit.
 *   - A NaN logit gives ce = NaN and a pred that is unspecified but inside [0, C).
 *   - meter[h] = [n, loss_sum, top1]: a second launch ADDS M, the sum of ce over the rows whose label is a class and the
 *     rows with pred == label.  One workgroup, fixed summation order, no atomics.
 *   Errors, all before any launch: VTX_ERR_NULL (x, labels, w, lse, ce, pred), VTX_ERR_SHAPE (M < 1, M > N, N >= 2^31, H
 *   outside 1..32, C < 1, H * C * D >= 2^31, D > 1024), VTX_ERR_ALIGN (D % 8 != 0; x or w not 16-byte aligned),
 *   VTX_ERR_DTYPE.
 *
 * vtx_probe_bwd: lse [H, M] of the forward; dw [H, C, D] fp32, db [H, C] fp32 (written, not added to).
 *   g = (__expf(logit - lse_row) - [c == label_row]) * scale in fp32 on the recomputed logits (a label outside [0, C)
 *   matches no class); dw[h, c, :] = sum over the rows of g x_row through a second MFMA, g rounded to bf16 (round to nearest
 *   even) on the way in bf16 mode; db[h, c] = sum of the unrounded g.  dX is not computed: the features are frozen.
 *   Rows are cut into slabs that fill the chip; the slab count is a function of (M, H, C, D) alone, the slabs' partials go
 *   to the workspace and are reduced in a fixed slab order: ascending.  vtx_probe_workspace_bytes(M, H, C, D) = slabs *
 *   (H C D + H C) * 4 bytes, 0 for one slab; ws may be NULL when that is 0.
 *   Errors: as the forward, and VTX_ERR_NULL (lse, dw, db; ws when a workspace is needed), VTX_ERR_SHAPE (scale not finite
 *   or not > 0), VTX_ERR_WORKSPACE (ws_bytes short).
 *
 * vtx_probe_sgd: one launch over all heads, torch.optim.SGD semantics (dampening 0, no Nesterov, buffers zero at the start):
 *     d = g + wd_h * w;   buf = mu * buf + d;   w = w - lr_h * buf
 *   on the fp32 masters w [H, C, D] / b [H, C] with momentum buffers mw / mb and gradients dw / db; the bias takes the same
 *   update with wd_h.  Contraction is off: every product and sum is rounded on its own in fp32, so a numpy float32
 *   restatement gives the same bits.  lr, wd: HOST arrays of H floats, copied into the launch.  shadow [H, C, D] bf16 or
 *   NULL: the round-to-nearest-even of the new master weights, written in the same pass (the w the next bf16 forward
 *   reads); in fp32 mode the shadow is the master itself and the pointer is NULL.
 *   Errors: VTX_ERR_NULL (any pointer but shadow), VTX_ERR_SHAPE (H outside 1..32, C < 1, D > 1024, H * C * D >= 2^31, mu
 *   outside [0, 1), a negative or non-finite lr or wd), VTX_ERR_ALIGN (D % 8 != 0). */
size_t vtx_probe_workspace_bytes(int64_t M, int H, int C, int D);
int vtx_probe_fwd(const void* x, const int32_t* rows, const int64_t* labels, const void* w, const float* bias, float* lse,
                  float* ce, int32_t* pred, double* meter, int64_t M, int64_t N, int H, int C, int D, int dtype,
                  void* stream);
int vtx_probe_bwd(const void* x, const int32_t* rows, const int64_t* labels, const void* w, const float* bias,
                  const float* lse, float* dw, float* db, int64_t M, int64_t N, int H, int C, int D, float scale, void* ws,
                  size_t ws_bytes, int dtype, void* stream);
int vtx_probe_sgd(float* w, float* b, float* mw, float* mb, const float* dw, const float* db, void* shadow, const float* lr,
                  const float* wd, float mu, int H, int C, int D, void* stream);

/* ---- Attention maps and per-head attention statistics (csrc/attention_maps.hip): read-only inspection of global attention.
 * The reference's attention probabilities are an ordinary tensor (models/vit.py:36-39); here no kernel stores them, so these
 * entries recompute them from the operands of vtx_attn_hd_fwd: q [B * Lq, nH * D] with row stride ldq, k [B * Lk, nH * D] with
 * row stride ldkv (the packed QKV projection, or the q | kv pair of PVT / Twins), bf16 or fp32, D a multiple of 8 in 8..128, any
 * Lq and Lk, scale = 1 / sqrt(D) formed as the attention kernels form it.  No bias, no mask, no windows.  No floating-point
 * atomics; the same inputs give the same bits.
 *
 * Scores: s = acc * scale, acc the MFMA chain of the attention kernels (v_mfma_f32_16x16x32_bf16, or the exact 16x16x4_f32 chain
 * in fp32; fp32 accumulation), one fp32 multiply.  Both score entries take the row maximum m in a first pass over the keys and
 * every sum against that final m in a second (K is re-read from L2; nothing is rescaled), each of a query's four lanes summing
 * its keys in ascending order and the four meeting in one fixed butterfly -- the term-by-term arithmetic is in the header comment
 * of csrc/attention_maps.hip.  A row's outputs are the same bits however the rows are cut into calls, however the batch is cut,
 * and whether the operand is the packed projection or a copy split into q and k.
 *
 * vtx_attn_map_rows: query rows row0 .. row0 + nrows - 1 of every image and head.  p fp32 [B, nH, nrows, Lk] = __expf(s - m) / l
 *   with l the row sum of __expf(s - m); lse fp32 [B, nH, nrows] = m + __logf(l).  row0 = 0, nrows = 1: the CLS map; row0 = 0,
 *   nrows = Lq: the whole P.
 * vtx_attn_map_stats: stats fp32 [B, nH, Lq, 5] per query row i, P never written:
 *     [0] lse                                                   bit-equal to the lse of vtx_attn_map_rows for that row
 *     [1] entropy = lse - (sum_j e_j s_j) / l                   in nats; e_j = __expf(s_j - m)
 *     [2] smax = m                                              the largest scaled logit, exact
 *     [3] prefix = (sum_{j < n_prefix} e_j) / l                 the mass on the CLS / prefix keys
 *     [4] dist = (sum_{j >= n_prefix} e_j |pos_i - pos_j|) / l  in patch units; token t >= n_prefix sits at ((t - n_prefix) / gw,
 *         (t - n_prefix) % gw); |.| is v_sqrt_f32 of the exact integer dy^2 + dx^2.  Mass on prefix keys counts as distance 0; a
 *         prefix query row stores 0; gh = gw = 0 switches dist off (0 is stored).  Keys and queries share the grid: gh * gw must
 *         equal Lk - n_prefix and Lq - n_prefix, so the q | kv pair of a sub-sampled attention runs with gh = gw = 0.
 * vtx_attn_map_meter: adds a stats tensor to meter fp64 [n_layer, nH, 6] at `layer`, one workgroup, fixed order: per head
 *   [queries, sum entropy, sum prefix, sum dist over the patch queries (i >= n_prefix), patch queries, max smax].  The last is a
 *   running maximum: the caller initialises it to -inf.  layer < n_layer is the caller's to keep.
 * vtx_attn_mass_mask: the thresholding of DINO's attention visualisation on n_maps fp32 maps of n <= 4096 values (below zero or
 *   NaN: counted as 0).  Sort ascending by (value, index): among equal values the lower index first.  The running sum in that
 *   order, in fp32, in chunks of 16 sorted elements: inside chunk c left to right, w[c][0] = v[16 c], w[c][i] = w[c][i - 1] +
 *   v[16 c + i]; P[0] = 0, P[c] = P[c - 1] + w[c - 1][15]; run[16 c + i] = P[c] + w[c][i]; total = run[n - 1];
 *   thr = (1.f - keep) * total in fp32.  Element e gets byte 1 iff run at its sorted position > thr, else 0: a sum that hits thr
 *   exactly is not kept and an all-zero map keeps nothing.  DINO's script divides by the total before the running sum; this
 *   does not: the only difference.
 *
 * Errors, all before any launch, with the codes of the vtx_attn_hd entries: VTX_ERR_NULL (any pointer), VTX_ERR_DTYPE,
 * VTX_ERR_SHAPE (B, Lq, Lk, nH, nrows, n_maps or n < 1; D outside the multiples of 8 in 8..128; B * Lq or B * Lk >= 2^31 - 1;
 * row0 < 0 or row0 + nrows > Lq; a stride below nH * D; n_prefix outside 0..min(Lq, Lk); gh, gw not both 0 and gh * gw !=
 * Lk - n_prefix or != Lq - n_prefix; layer < 0; n > 4096; keep outside (0, 1]), VTX_ERR_ALIGN (a stride that is not a multiple of
 * 8; q or k off 16 bytes; an fp32 pointer off 4, the meter off 8). */
int vtx_attn_map_rows(const void* q, const void* k, int64_t ldq, int64_t ldkv, float* p, float* lse, int B, int Lq, int Lk, int nH,
                      int D, int row0, int nrows, int dtype, void* stream);
int vtx_attn_map_stats(const void* q, const void* k, int64_t ldq, int64_t ldkv, float* stats, int B, int Lq, int Lk, int nH, int D,
                       int n_prefix, int gh, int gw, int dtype, void* stream);
int vtx_attn_map_meter(const float* stats, double* meter, int layer, int B, int nH, int Lq, int n_prefix, void* stream);
int vtx_attn_mass_mask(const float* maps, uint8_t* mask, int n_maps, int n, float keep, void* stream);

/* ---- Attention maps and statistics for window and halo attention (csrc/attention_maps.hip, template flag WX): what
 * vtx_attn_map_rows / vtx_attn_map_stats give for global attention, for the layers of Swin, the Twins locally-grouped half and
 * Halo (reference models/swin_transformer.py:103-160, where `attn` is an ordinary tensor).  The entries above keep their bits.
 *
 * Operands exactly as vtx_attn_hdw_fwd takes them.  win > 0: B images, q / k the packed projection of the (H, W) map in map
 * order; token t of window n of image b is found by the rolled address (shift != 0: the roll by -win / 2); Lq == Lk == win * win;
 * problems = B * nW.  win == 0: B problems of plain rows (the gathered q | kv pair of halo attention, or a packed projection);
 * H, W, shift are ignored.  bias fp32 [nH][Lq][Lk] or NULL; mask uint8 [nW][Lq][Lk] or NULL (nonzero: the cell is excluded;
 * win > 0 only).  Precondition, as in vtx_attn_hdw_fwd: every query row keeps at least one unmasked key; a key block that is
 * fully masked for a query is fine (the maximum is final before any exponential is taken: no -inf - -inf can appear).
 *
 * Scores: a = acc * scale as above (the rounded product); with a bias s = a + bias[h][i][j], a separate fp32 add that is never
 * contracted with the product; without a bias s = a.  A masked cell and a key >= Lk are excluded: never in the maximum, e = 0
 * exactly, nothing added to any sum (the entropy term e * s is skipped, not formed).  Passes, lane order and butterfly as above.
 *
 * vtx_attn_mapw_rows: p fp32 [problems, nH, nrows, Lk] (a masked cell exactly 0.f), lse fp32 [problems, nH, nrows].
 * vtx_attn_mapw_stats: stats fp32 [problems, nH, Lq, 5] in the (problem, head, query) order of vtx_attn_hdw_fwd's lse:
 *     [0] lse = m + __logf(l)                                   bit-equal to the lse of vtx_attn_mapw_rows for that row
 *     [1] entropy = lse - (sum over unmasked j of e_j s_j) / l
 *     [2] smax = m                                              the largest score that enters the softmax: bias included, masked
 *                                                               keys excluded; exact as a maximum
 *     [3] self = e_self / l                                     the mass on the query's own token
 *     [4] dist = (sum_j e_j |pos_i - pos_j|) / l                in token units; |.| is v_sqrt_f32 of the exact integer dy^2 + dx^2
 *   Window mode: token t sits at (t / win, t % win) of its window, queries and keys alike; self is key j == i; gq, gk ignored
 *   (pairs the shifted partition brings together across the map edge are masked, so window coordinates are true distances for
 *   every cell that counts).  Halo mode (win == 0): query t sits at (off + t / gq, off + t % gq) of the key grid of width gk,
 *   off = (gk - gq) / 2; key j at (j / gk, j % gk); self is the key at the query's own position; gq = gk = 0 switches self and
 *   dist off (0 is stored).  Slot 3 sits where the prefix mass sits: vtx_attn_map_meter with n_prefix = 0 sums
 *   [queries, sum entropy, sum self, sum dist, queries, max smax] from this tensor.
 * With win == 0, bias == NULL, mask == NULL and gq = gk = 0, p, lse and slots 0..2 are bit-equal to vtx_attn_map_rows /
 * vtx_attn_map_stats on the same operands.  A row's outputs are the same bits however the images are cut into calls and however
 * row0 / nrows cut the rows.  No floating-point atomics.
 *
 * Errors, all before any launch, with the codes of the vtx_attn_hdw and vtx_attn_map entries: VTX_ERR_NULL (q, k or an output),
 * VTX_ERR_DTYPE, VTX_ERR_SHAPE (B, Lq, Lk, nH or nrows < 1; D outside the multiples of 8 in 8..128; row0 < 0 or row0 + nrows >
 * Lq; a stride below nH * D; win < 0; H or W not a positive multiple of win; Lq != win * win or Lk != Lq with win > 0; a mask with
 * win == 0; in halo mode with gq, gk not both 0: gq * gq != Lq, gk * gk != Lk, gk < gq or gk - gq odd; problems * Lq >= 2^31 - 1;
 * nH * Lq * Lk >= 2^31 - 1), VTX_ERR_ALIGN (a stride that is not a multiple of 8; q or k off 16 bytes; an fp32 pointer off 4). */
int vtx_attn_mapw_rows(const void* q, const void* k, int64_t ldq, int64_t ldkv, float* p, float* lse, const float* bias,
                       const uint8_t* mask, int B, int Lq, int Lk, int nH, int D, int H, int W, int win, int shift, int row0,
                       int nrows, int dtype, void* stream);
int vtx_attn_mapw_stats(const void* q, const void* k, int64_t ldq, int64_t ldkv, float* stats, const float* bias,
                        const uint8_t* mask, int B, int Lq, int Lk, int nH, int D, int H, int W, int win, int shift, int gq, int gk,
                        int dtype, void* stream);

/* ---- Weighted column sums of P (csrc/attention_maps.hip): the primitive of attention rollout -- a row vector pushed through
 * A_l = residual I + (1 - residual) mean_h P_l, layer by layer -- and of the mean attention a key token receives.  The entries
 * above keep their bits and their code.
 *
 * Operands: q, k, ldq, ldkv, B, Lq, Lk, nH, D, dtype exactly as vtx_attn_map_rows takes them (bf16 or fp32, D a multiple of 8 in
 *   8..128, the packed projection or the q | kv pair by pointer and stride).  w fp32 [B, R, Lq], 1 <= R <= 16, shared by the
 *   heads; any finite values, negative ones included.
 * Probabilities: s, m, l and p_ij = __expf(s_ij - m_i) / l_i are formed as vtx_attn_map_rows forms them -- the same passes, the
 *   same lane order, the same butterfly, the IEEE division: p_ij is bit for bit the value that entry stores.
 * Column sums: t = w[b, r, i] * p_ij is one fp32 product, rounded on its own (never one fma with the add); c[b, h, r, j] is the
 *   fp32 sum of t over i in an order that depends on Lq alone, not on B, R, the launch geometry or the other weight rows of the
 *   call: queries in tiles of 16; wave v of 4 adds, per query lane i % 16, its tiles v, v + 4, v + 8, .. in ascending order from
 *   0.f; the 16 query lanes meet in one fixed butterfly; the four waves are added in wave order.  c is stored to out_heads fp32
 *   [B, nH, R, Lk], or kept in the workspace when out_heads is NULL.
 * Blend: out_mix fp32 [B, R, Lk] (optional; needs Lq == Lk) = (alpha * w[b, r, j]) + (beta * (c_0 + c_1 + .. + c_{nH-1})), the
 *   heads summed in ascending order, every product and sum one fp32 operation in that written order, none contracted into an
 *   fma.  At least one of out_heads and out_mix is non-NULL.
 * Bits: an image's outputs are the same bits however the batch is cut into calls; a weight row's whatever other rows share the
 *   call; the same for the packed projection and a split copy, and for either output asked for alone or both.  A zero weight
 *   contributes an exact zero, so a one-hot weight row w = e_i makes out_heads[b, h, r, :]
 *   bit-equal to the row vtx_attn_map_rows stores for query i (and 2^-3 e_i to that row times 2^-3); alpha = 1, beta = 0
 *   returns w.
 * P is never written: no buffer of Lq * Lk exists per problem.  The workspace holds (m, l) per query and room for c:
 *   vtx_attn_map_colsum_workspace_bytes = 4 * (2 B nH Lq + B nH R Lk) bytes (0 for sizes the entry refuses).  Three launches on
 *   `stream`: (m, l); the column sums; the blend (only with out_mix).  No floating-point atomics.
 *
 * Errors, all before any launch, with the codes of the vtx_attn_map entries: VTX_ERR_NULL (q, k, w, or both outputs NULL),
 * VTX_ERR_DTYPE, VTX_ERR_SHAPE (B, Lq, Lk or nH < 1; D outside the multiples of 8 in 8..128; R outside 1..16; out_mix with
 * Lq != Lk; a stride below nH * D; B * Lq or B * Lk >= 2^31 - 1; alpha or beta not finite), VTX_ERR_ALIGN (a stride that is not a
 * multiple of 8; q or k off 16 bytes; an fp32 pointer or the workspace off 4), VTX_ERR_WORKSPACE (ws NULL or ws_bytes short). */
size_t vtx_attn_map_colsum_workspace_bytes(int B, int Lq, int Lk, int nH, int R);
int vtx_attn_map_colsum(const void* q, const void* k, int64_t ldq, int64_t ldkv, const float* w, float* out_heads, float* out_mix,
                        float alpha, float beta, int B, int Lq, int Lk, int nH, int D, int R, void* ws, size_t ws_bytes, int dtype,
                        void* stream);

/* ---- Label propagation for semi-supervised video object segmentation on frozen patch tokens (csrc/labelprop.hip,
 * csrc/knn_select.h): the DAVIS protocol of the DINO paper.  The search is vtx_knn_topk restricted to a spatial
 * neighbourhood by address arithmetic; no affinity matrix of n_ctx P x P exists and no score outside the neighbourhoods is
 * formed.  No host synchronisation, no floating-point atomics: the same inputs give the same bits.
 *
 * Geometry: B independent sequences on a patch grid h x w; token p = y * w + x, P = h w; feature width D.
 *
 * vtx_labelprop_topk: tar [B, P, D] the target frame, ctx [B, S, P, D] a ring of S frame slots, both dtype (bf16 / fp32);
 *   rows are used as given -- nothing is normalised here.  slots: HOST array of n_ctx (1..16) slot numbers in 0..S-1, copied
 *   into the launch by value (no device copy, no synchronisation: rotating the queue is free); a slot may repeat.
 *   - Candidates.  Key (c, p') is token p' of slot slots[c]; its index is c * P + p'.  It is a candidate for query (y, x)
 *     exactly when |y - y'| <= radius and |x - x'| <= radius: a Chebyshev box clipped at the grid border, with no wrap from
 *     one grid row into the next.  radius >= max(h, w) - 1 restricts nothing.
 *   - val [B, P, k] fp32, idx [B, P, k] int32: the first k candidates in the total order of vtx_knn_topk -- higher score
 *     first, among equal scores the lower index first -- listed in that order.  A query with fewer than k candidates ends
 *     its list with the sentinels (-inf, 0x7fffffff).
 *   - Exactly k under a total order.  The usual torch composition (dense exp(f_tar . f_ctx / T), a box mask, topk, a
 *     threshold at the k-th largest weight) keeps EVERY key whose weight is >= the k-th largest; this entry keeps exactly
 *     k.  The two differ on exact ties at the k-th place, and only there.
 *   - Pair-local scores.  The score of a pair is the fp32 result of ONE MFMA chain over D that depends on its two rows
 *     only: v_mfma_f32_16x16x32_bf16 per 32 columns (bf16) or 8 x v_mfma_f32_16x16x4_f32 per 32 columns (fp32, exact
 *     products), chunks ascending from 0.f -- the chain of vtx_knn_topk, so a pair's val is bit for bit what vtx_knn_topk
 *     returns for the same two rows.  A query's list does not depend on B, on how the batch is cut into calls, or on
 *     which tile the query falls in.
 *   - A NaN score orders as -inf.  Every written index is a real candidate index or the sentinel, and the call ends.
 *   Errors, all before any launch, with the codes of the k-NN entries: VTX_ERR_NULL (tar, ctx, slots, val, idx),
 *   VTX_ERR_SHAPE (B, h, w < 1; n_ctx outside 1..16; a slot outside 0..S-1; D > 1024; k outside 1..64; radius < 0;
 *   n_ctx * P >= 2^31 - 1; B * S * P >= 2^31), VTX_ERR_DTYPE, VTX_ERR_ALIGN (D % 8 != 0; tar or ctx not 16-byte aligned; val
 *   or idx off 4).
 *
 * vtx_labelprop_vote: val / idx [B, P, k] (a search result), seg [B, S, P, C] fp32 the soft labels of the ring, channels
 *   last, slots / n_ctx / S as above, out [B, P, C] fp32, temperature T.  Per query, i over the k places in order:
 *     d_i    = val_i - val_0              one fp32 subtraction; val_0 = the list's first score, its largest; d_i = 0 where
 *                                         val_i == val_0 (so that -inf - -inf is not formed)
 *     w_i    = expf(d_i / T)              one fp32 division, expf; w_0 = 1 and no w_i can overflow.  After the
 *                                         normalisation below this is the composition's exp(val_i / T).
 *     num[c] = sum_i (w_i * seg[key_i][c])   each product one fp32 multiply rounded on its own, added in neighbour order
 *     den    = sum_i w_i                     added in neighbour order
 *     out[c] = num[c] / den               one IEEE fp32 division; 0 where no place counts
 *   Products and sums are never contracted into an fma.  key_i = (slot slots[idx_i / P], token idx_i % P).  A sentinel place
 *   is skipped: it adds to neither sum.  So is any other index outside [0, n_ctx P): it is refused by nothing on the device,
 *   it is skipped and never dereferenced.
 *   Errors, all before any launch: VTX_ERR_NULL (any pointer), VTX_ERR_SHAPE (C outside 1..1024; k outside 1..64; T not > 0
 *   or not finite; B, P < 1; n_ctx outside 1..16; a slot outside 0..S-1; n_ctx * P >= 2^31 - 1; B * S * P >= 2^31),
 *   VTX_ERR_ALIGN (a pointer off 4).
 *
 * vtx_mask_overlap: pred, gt [N, P] int32 label maps; counts [N, C, 3] int64 = per map and per label c in [0, C):
 *   [#(pred == c & gt == c), #(pred == c), #(gt == c)].  Labels outside [0, C) count for nothing.  Integer, fixed order, no
 *   atomics; counts is overwritten.  The region similarity J of a label is inter / (|pred| + |gt| - inter).
 *   Errors, all before any launch: VTX_ERR_NULL, VTX_ERR_SHAPE (N, P, C < 1; C > 256; N * P >= 2^31), VTX_ERR_ALIGN (pred or
 *   gt off 4, counts off 8). */
int vtx_labelprop_topk(const void* tar, const void* ctx, const int32_t* slots, int n_ctx, int S, float* val, int32_t* idx,
                       int64_t B, int h, int w, int D, int radius, int k, int dtype, void* stream);
int vtx_labelprop_vote(const float* val, const int32_t* idx, const float* seg, const int32_t* slots, int n_ctx, int S,
                       float* out, int64_t B, int64_t P, int k, int C, float T, void* stream);
int vtx_mask_overlap(const int32_t* pred, const int32_t* gt, int64_t* counts, int64_t N, int64_t P, int C, void* stream);

/* ---- Multi-tensor weight cast (csrc/cast.hip): all fp32 Linear / Conv weights of a model -> bf16, plain [out][in]
 * and transposed [in][out], in one launch per forward.  This is the per-call weight cast of the reference's bf16
 * autocast (torch.cuda.amp.autocast around model(input), train.py:273-274) done once for the whole model.
 * desc: device array of nmat records {const float* src; int64 off; int rows, cols, tile0, tiles_c}
 * (vtx_cast_desc_bytes() each); ntiles = sum ceil(rows/64)*ceil(cols/64); matrix i occupies
 * [off_i, off_i + rows_i*cols_i) of both flat bf16 outputs. */
size_t vtx_cast_desc_bytes(void);
int vtx_cast_weights(const void* desc, int nmat, int ntiles, void* dst, void* dst_t, void* stream);

/* ---- Patch gather: NCHW fp32 image -> patch matrix [B*(H/p)*(W/p), Kp] of dtype, columns >= 3*p*p zero.
 *   order 0: column (py, px, c)  -- Swin: permute(0,2,3,1) + patchify(4) (models/swin_transformer.py:15-22,
 *            208-213, 371); the Linear(48, C) then runs as vtx_gemm on the padded K = Kp
 *   order 1: column (c, py, px)  -- ViT: Conv2d(3, C, p, stride=p) as an im2col GEMM (models/vit.py:73, 76) */
int vtx_patch_gather(const float* x, void* out, int B, int Cin, int H, int W, int p, int Kp, int order, int dtype,
                     void* stream);
/* Same patch matrix from a bf16 NHWC image [B, H, W, Cin] (vtx_mix_normalize_erase's out_nhwc_bf16 output), W % 8 == 0. */
int vtx_patch_gather_nhwc(const void* x, void* out, int B, int Cin, int H, int W, int p, int Kp, int order, int dtype,
                          void* stream);
/* ---- Token mean over Tn tokens: AdaptiveAvgPool2d(1)+Flatten of the Swin classifier
 * (models/swin_transformer.py:281, 376-377) on NHWC features. */
int vtx_token_mean_fwd(const void* x, void* y, int B, int Tn, int C, int dtype, void* stream);
int vtx_token_mean_bwd(const void* dy, void* dx, int B, int Tn, int C, int dtype, void* stream);
/* ---- ViT token assembly (models/vit.py:140-143): out[b,0] = cls + pos[0]; out[b,1+t] = patches[b,t] + pos[1+t].
 * L = n_patch + 1; cls [C], pos [L, C] fp32.  Backward: dpatches, dcls [C], dpos [L, C] (fp32, batch sums). */
int vtx_vit_assemble_fwd(const void* patches, const float* cls, const float* pos, void* out, int B, int L, int C,
                         int dtype, void* stream);
int vtx_vit_assemble_bwd(const void* dx, void* dpatches, float* dcls, float* dpos, int B, int L, int C, int dtype,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTX_H_ */
