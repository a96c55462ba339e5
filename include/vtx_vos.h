/* vtx_vos.h -- second public header of libvtx.so: the DAVIS-2017 J&F evaluation on the device (csrc/davis.hip, vtx.vos).
 *
 * vtx.h stays the statement of the entries it declares; this file declares the entries that turn the soft labels of
 * vtx_labelprop_vote into label maps and count the pixels behind the boundary measure F.  csrc/vtx_common.h includes it after
 * vtx.h, so every translation unit compiles against these prototypes, and vtx/_lib.py binds the library from this file the way
 * it binds vtx.h (a table of its own; VTX_VOS_ABI_VERSION against vtx_vos_abi_version()).  The conventions are vtx.h's: 0 or a
 * negative VTX_ERR_* code of vtx.h (vtx_strerror serves them; no code is defined here), device pointers owned by the caller,
 * kernels enqueued on `stream`, no host synchronisation, no floating-point atomics: the same inputs give the same bits.
 */
#ifndef VTX_VOS_H_
#define VTX_VOS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header's entries (bumped on any signature change here; VTX_ABI_VERSION of vtx.h does not move with it). */
#define VTX_VOS_ABI_VERSION 1
int vtx_vos_abi_version(void);

#define VTX_VOS_MAX_LABELS 256   /* channels vtx_seg_labels takes at most: the label range of vtx_mask_overlap */
#define VTX_VOS_MAX_SCALE 32     /* largest integer upsampling factor */
#define VTX_VOS_MAX_OBJECTS 255  /* objects vtx_boundary_counts counts at most (labels 1..255) */
#define VTX_VOS_MAX_RADIUS 32    /* largest dilation radius */
#define VTX_VOS_BAND_ROWS 64     /* rows of one workgroup's band in the dilation launch: H = 65 is the first two-band map */

/* ---- vtx_seg_labels: soft labels on the patch grid -> integer label map, DINO's eval_video_segmentation pipeline in its order.
 * seg [N, C, gh, gw] fp32 contiguous (propagate_video's output with B T flattened); labels [N, oh, ow] int32;
 * H = gh scale, W = gw scale; oh = ow = 0 means (H, W).
 *
 * 1. Bilinear upsample, the rule of F.interpolate(scale_factor = scale, mode = "bilinear", align_corners = False).  Output
 *    index d = scale q + r on an axis of n grid points: f = (r + 0.5) / scale - 0.5 (double, on the host; a function of r
 *    alone); f >= 0: i0 = q, l1 = f, otherwise i0 = q - 1, l1 = 1 + f; i0 < 0: i0 = 0, l1 = 0; i1 = min(i0 + 1, n - 1); l1 is
 *    rounded to fp32 once and l0 = 1.0f - l1 is an fp32 subtraction.  The value is
 *        u = l0y * (l0x * v00 + l1x * v01) + l1y * (l0x * v10 + l1x * v11)
 *    with every product and every sum rounded to fp32 on its own, in the order written; nothing is contracted into an fma.
 * 2. normalize != 0: mn, mx = the minimum and the maximum of u over the whole H x W map of channel (n, c) -- the computed
 *    values, not the grid's (with an even scale no sample coincides with a grid point off the clamped border).  A map that
 *    holds a NaN has mn = mx = NaN.  Where mx > 0 and mx != mn: u' = (u - mn) / (mx - mn), one fp32 subtraction each and one
 *    correctly rounded fp32 division; otherwise the channel is left as it is.
 * 3. Argmax over c: the lower channel wins among equal values, a NaN never wins, a pixel whose values are all NaN gets 0.
 * 4. Nearest resize: labels[n, i, j] is the label of the upsampled pixel (((2 i + 1) H) div (2 oh), ((2 j + 1) W) div (2 ow)),
 *    in integer arithmetic (the pixel-centre rule; PIL's resize(NEAREST) forms the index in floating point and differs from
 *    it in isolated columns, e.g. 1 of 854 for 848 -> 854).  Only these pixels are argmaxed; step 2 is over all H W pixels;
 *    the N C H W upsampled tensor is never written.
 * ws: vtx_seg_labels_workspace(N, C) bytes (2 N C 32-bit words: the extrema travel as integer atomics on the monotone bit
 *    pattern -- minimum and maximum are order-free); not read and may be NULL when normalize == 0.  The size is 0 for
 *    arguments the entry refuses.
 * Errors, all before any launch, with the codes of vtx_mask_overlap: VTX_ERR_NULL (seg, labels; ws when normalize != 0),
 *    VTX_ERR_SHAPE (N, C, gh, gw < 1; C > 256; scale outside 1..32; exactly one of oh, ow zero, or either negative;
 *    N C gh gw, N H W or N oh ow >= 2^31), VTX_ERR_ALIGN (a pointer off 4), VTX_ERR_WORKSPACE (ws_bytes short). */
size_t vtx_seg_labels_workspace(int64_t N, int C);
int vtx_seg_labels(const float* seg, int32_t* labels, int64_t N, int C, int gh, int gw, int scale, int oh, int ow,
                   int normalize, void* ws, size_t ws_bytes, void* stream);

/* ---- vtx_boundary_counts: the pixel counts behind the boundary measure F of davis2017-evaluation (f_measure, seg2bmap,
 * cv2.dilate with skimage.morphology.disk).  pred, gt [N, H, W] int32 label maps; counts [N, n_obj, 4] int64 =
 * (|b_pred|, |b_gt|, |b_pred & dil(b_gt)|, |b_gt & dil(b_pred)|) per map and per object c in 1..n_obj, overwritten.
 * Per object and map, m = (map == c); other labels count for nothing.
 *   boundary   b[y, x] = (m[y, x] != m[y, x+]) | (m[y, x] != m[y+, x]) | (m[y, x] != m[y+, x+]),
 *              x+ = min(x + 1, W - 1), y+ = min(y + 1, H - 1): seg2bmap's last row, last column and zero corner.
 *   dilation   dil(b)[y, x] = OR of b[y + dy, x + dx] over dx^2 + dy^2 <= radius^2; positions outside the map contribute 0
 *              (cv2.dilate's default border); radius 0 is the identity.
 * The counts are integer population counts (integer atomics over bands of VTX_VOS_BAND_ROWS rows: sums of integers are
 * order-free).  P = match_pred / |b_pred|, R = match_gt / |b_gt|, F = 2 P R / (P + R) are the caller's.
 * ws: vtx_boundary_workspace(N, n_obj, H, W) bytes = the bit rows [N, n_obj, 2, H, ceil(W / 64)] of 64-bit words; 0 for
 *    arguments the entry refuses.
 * Errors, all before any launch: VTX_ERR_NULL (any pointer), VTX_ERR_SHAPE (N, H, W, n_obj < 1; n_obj > 255; radius outside
 *    0..32; N H W >= 2^31), VTX_ERR_ALIGN (pred, gt off 4; counts, ws off 8), VTX_ERR_WORKSPACE (ws_bytes short). */
size_t vtx_boundary_workspace(int64_t N, int n_obj, int H, int W);
int vtx_boundary_counts(const int32_t* pred, const int32_t* gt, int64_t* counts, int64_t N, int H, int W, int n_obj,
                        int radius, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif  /* VTX_VOS_H_ */
