/*
 * ppms.h -- C ABI of libppms (MI355X / gfx950 kernels for the PPMStereo hot path).
 *
 * The reference (cocowy1/PPMStereo) has no native code: every op below replaces a PyTorch call site on the path
 * PPMStereo.forward_update_block (/root/reference/models/core/ppmstereo.py:426-594).  Each entry point cites the
 * reference interface it replaces.  Conventions:
 *   - plain pointers and sizes only; all pointers are DEVICE pointers owned by the caller (PyTorch caching
 *     allocator); the library never allocates, frees or retains device memory;
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*); no call synchronises the device;
 *   - return 0 on success, a negative PPMS_E* code otherwise; ppms_last_error() gives the thread-local message;
 *   - "SP" tensors are the library's internal activation format: channel-last [pixel][ld] bf16 hi plane and
 *     bf16 lo plane with x ~= hi + lo (fp32-accurate bf16x3 MFMA operands).  pixel = (frame*H + y)*W + x.
 */
#ifndef PPMS_H
#define PPMS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPMS_OK 0
#define PPMS_EINVAL (-1)   /* shape / argument contract violated (e.g. W too small for the pyramid) */
#define PPMS_ELAUNCH (-2)  /* HIP launch error */
#define PPMS_ENODEV (-3)   /* no gfx950 device */

#define PPMS_ABI_VERSION 4

int ppms_version(void);
const char* ppms_last_error(void);
/* 0 when a gfx950 device is current; fills name (<= 63 chars) */
int ppms_device_info(char* name, int name_cap, int* cu_count, int* clock_mhz);

/* ---------------------------------------------------------------- correlation (models/core/corr.py) */
/* CorrBlock1D.__init__ + CorrBlock1D.corr, corr.py:56-72,96-104.
 * fmap1,fmap2: fp32 NCHW (B,C,H,W).  pyr[l] (l=0..4): fp32 (B*H*W, W>>l) with W>>l floored; level 4 is stored
 * but never read, as in the reference.  vol = sum_c f1 f2 / sqrt(C); level l+1 = avg of adjacent pairs. */
int ppms_corr_build(const float* fmap1, const float* fmap2, float* const pyr[5], int B, int C, int H, int W, void* stream);

/* CorrBlock1D.__call__ + bilinear_sampler + coords_grid, corr.py:74-94,10-27,47-52.
 * flow: fp32, (B,2,H,W) NCHW when flow_nhwc == 0, [pixel][2] otherwise (only channel 0 is read).
 * out_nchw (optional): fp32 (B,36,H,W).  out_hi/out_lo (optional): SP [pixel][out_ld], channels 36..63 zeroed.
 * flow_sp_hi/lo (optional): SP copy of both flow channels written at [pixel][flow_sp_ld] + {0,1}. */
int ppms_corr_lookup(const float* const pyr[4], const float* flow, int flow_nhwc, float* out_nchw, void* out_hi, void* out_lo,
                     int out_ld, void* flow_sp_hi, void* flow_sp_lo, int flow_sp_ld, int B, int H, int W, void* stream);

/* ---------------------------------------------------------------- implicit-GEMM convolution */
/* Replaces every cuDNN conv2d/conv3d call of the update block (ppmtereo_update.py:292-310, 473-480, 673-674,
 * 889-893, 910-914, 646, 129): out[cout][pixel] = sum_{tap,ci} W[cout][tap][ci] * X[ci][pixel + tap], zero padded,
 * computed as hi*hi + hi*lo + lo*hi on bf16 MFMA with fp32 accumulation. */
typedef struct ppms_sp {          /* a channel-last split-bf16 view */
    void* hi;
    void* lo;
    int32_t ld;                   /* elements between pixels */
    int32_t c;                    /* channels in this view (inputs: multiple of 32) */
} ppms_sp;

enum {                            /* epilogue kinds */
    PPMS_EPI_STORE = 0,           /* y = act(acc + bias) * scale                                 */
    PPMS_EPI_RESID = 1,           /* y = act(aux_sp + acc + bias)                                  */
    PPMS_EPI_RH = 2,              /* y = sigmoid(acc + bias) * aux_sp               (GRU r * h)    */
    PPMS_EPI_GRU = 3,             /* y = (1 - z) * aux_sp + z * tanh(acc + bias), z = aux_f32      */
    PPMS_EPI_ADDF32 = 4           /* out_f32 += acc + bias (in place)              (flow += dflow) */
};
enum { PPMS_ACT_NONE = 0, PPMS_ACT_RELU = 1, PPMS_ACT_GELU = 2, PPMS_ACT_SIGMOID = 3, PPMS_ACT_TANH = 4, PPMS_ACT_ELU1 = 5 /* elu(x)+1 */ };

typedef struct ppms_epilogue {
    int32_t kind, act;
    float scale;
    int32_t n_valid;              /* couts [0, n_valid) of this half are stored                    */
    ppms_sp out_sp;               /* optional (hi == NULL: skip)                                   */
    float* out_f32;               /* optional [pixel][out_f32_ld]                                  */
    int32_t out_f32_ld;
    int32_t vt_f16;               /* format of out_vt: 0 = bf16(y); 1 = the fp16 image of bf16(y), saturated at +-65504 -- the same numbers
                                   * (every bf16 value of magnitude 2^-14 .. 65504 is an fp16 value; below, fp16 subnormals keep 2^-25 absolute)
                                   * in the operand format of ppms_mem_attn's PPMS_ATTN_P_FP16 mode.  (Sits in what was padding: ABI size unchanged.) */
    void* out_vt;                 /* optional 16-bit [frame][n_valid][H*W] (transposed, attention V), format: vt_f16 */
    ppms_sp aux_sp;               /* residual / h                                                  */
    const float* aux_f32;         /* z                                                             */
    int32_t aux_f32_ld;
    int32_t pre_f32_ld;
    const float* pre_f32;         /* optional [pixel][pre_f32_ld]: added to acc + bias before the activation -- the
                                   * contribution of input channels that do not change between iterations (computed
                                   * once per scale by another launch of the same conv on those channels)         */
} ppms_epilogue;

typedef struct ppms_conv {
    ppms_sp seg[2];               /* input channel segments, concatenated along K                 */
    int32_t nseg;
    int32_t groups;               /* 0 / 1: every cout reads all input channels (the segments concatenated along K).  2: a GROUPED convolution of two
                                   * groups -- nseg == 2, input segment s feeds the couts of epilogue half s only (couts [0, m_split) read seg[0], couts
                                   * [m_split, M) read seg[1]; weights: the two convolutions' packed images interleaved per k-step, pack_conv6_grouped).
                                   * Served by ppms_conv_gemm6 only (ppms_conv_gemm6_applicable tells); every other entry point refuses it.
                                   * (Sits in what was padding: ABI size unchanged.) */
    const void* w;                /* packed weights, see ppmstereo_amd/packing.py                  */
    const float* bias;            /* [M] fp32 (never NULL; zeros when the conv has no bias)        */
    int32_t T, H, W;              /* volume; pixels = T*H*W                                        */
    int32_t kt, kh, kw;           /* odd kernel extents, "same" zero padding                       */
    int32_t M;                    /* padded couts, multiple of 64                                  */
    int32_t m_split;              /* couts >= m_split use epi[1] with cout - m_split (multiple of 64; >= M: unused) */
    int32_t t_halo;               /* frames that exist (and may be read by temporal taps) before frame 0 and after frame T-1 of
                                   * every input segment: 0 = zero padding at both ends (one GPU holds the whole window); > 0 when
                                   * the window's frames are sharded over GPUs and the neighbours' boundary frames sit in halo
                                   * slabs around this rank's T frames (ppmstereo_amd/dist.py).  Outputs cover [0, T) only. */
    int32_t lo_zero_from;         /* > 0: the input channels from this index on (counted over the concatenated segments; a multiple of
                                   * 64) are known to hold bf16-exact values, i.e. their lo plane is all zero (the memory read-out `hid` of
                                   * the attention, ppmstereo.py:550-552, is a bf16 tensor): the kernels skip the products with that plane
                                   * -- the same bits, a third of those channels' MFMAs saved.  A PROMISE by the caller: with a non-zero
                                   * lo plane there the result silently loses that plane's contribution.  0: no such channels. */
    ppms_epilogue epi[2];
} ppms_conv;

/* desc: host copy (validated, sizes the grid, and -- since ABI v2 -- copied into the kernel arguments at launch, so it may be
 * changed or freed as soon as the call returns); dev_desc: the same bytes in device memory (caller-owned; must be non-NULL, kept in
 * the signature for ABI stability: the kernels no longer read it -- a descriptor in the kernel arguments saves a dependent memory
 * round trip at the head of every launch and is known not to alias the kernel's stores).
 *
 * THE CONTRACT OF THE RATINGS.  Every kernel below has a rating function (*_applicable, *_slices) next to its launch entry point, and both
 * run the same descriptor check (csrc/conv_check.h) and the same geometry planner: a non-zero rating, plus a descriptor that passes the
 * operand tier, means the launch entry point returns 0 -- called with the library's own choice of hints (0) and, for the sliced forms, the
 * returned slice count.  The check has two tiers.  Shape / addressing tier, what a rating relies on: nseg 1..2, groups, a volume > 0,
 * t_halo 0..8, odd taps within the kernel's maxima, M / m_split, per segment non-NULL 16-byte-aligned planes, c a multiple of the
 * kernel's chunk, ld % 8 == 0, and whether the kernel serves out_vt / PPMS_EPI_ADDF32.  Operand tier, what only a launch needs: w and
 * bias, and per live epilogue half n_valid > 0, a known kind, the operands of that kind and their alignment (16 bytes; ld % 8 == 0 for SP
 * views, % 4 for fp32).  ppms_conv_gemm2 / 5 / 6 ratings never look at the operand tier; ppms_gemm1_applicable and
 * ppms_conv_stream_applicable check both.  A refusal leaves "<kernel>: <field>=<value> ..." in ppms_last_error(). */
/* Data-reuse tiling: all couts of a pixel tile per workgroup, LDS activation window swept by the kw taps.
 * desc->w must be in the pack_conv2 layout (ppmstereo_amd/packing.py); segments in multiples of 32 channels, M a multiple of 64, kw <= 15.
 * wm_hint: 64-cout blocks per workgroup (1..4), 0 = let the library choose from the grid size. */
int ppms_conv_gemm2(const ppms_conv* desc, const ppms_conv* dev_desc, int wm_hint, void* stream);
/* K-sliced form of the same kernel for small maps (1/16 and 1/8 scales: fewer workgroups than CUs, long K loops):
 * nslice workgroups share each output tile and leave fp32 partial sums in `workspace` (caller-owned,
 * ppms_conv_gemm2_slice_workspace_bytes() bytes), a second launch sums them in slice order (deterministic) and runs the
 * fused epilogue.  ppms_conv_gemm2_slices() returns the slice count that pays off for a descriptor (1: use
 * ppms_conv_gemm2 -- also for what the kernel does not serve).  Not for epilogues with out_vt. */
int ppms_conv_gemm2_slices(const ppms_conv* desc);
int64_t ppms_conv_gemm2_slice_workspace_bytes(const ppms_conv* desc, int nslice);
int ppms_conv_gemm2_sliced(const ppms_conv* desc, const ppms_conv* dev_desc, int nslice, void* workspace, void* stream);
/* Convs with kh > 1 by the same kernel with ONE halo'd window per (dt, chunk) for all their taps (ppms_conv_gemm2 loads a
 * window per kernel row): (kt, kh, 1) kernels swept along y (weights: pack_conv2 order with the kh / kw axes swapped),
 * kernels with kw > 1 as well through a 2-D window (weights: (ky, kx) flattened into x) -- the sweep-ordered packs
 * ppms_conv_gemm5 / ppms_conv_gemm6 use too.  nslice / workspace as for ppms_conv_gemm2_sliced (nslice == 1: none);
 * ppms_conv_gemm2_ysweep_slices() = the slice count that pays off (0: not a candidate / window does not fit). */
int ppms_conv_gemm2_ysweep_slices(const ppms_conv* desc);
int ppms_conv_gemm2_ysweep(const ppms_conv* desc, const ppms_conv* dev_desc, int nslice, void* workspace, void* stream);
/* Barrier-free k-loop (conv_gemm5.hip): the weights are packed in MFMA-fragment order (ppmstereo_amd/packing.py pack_conv4,
 * sweep-ordered: y-swept kernels with kh / kw swapped, 2-D swept ones with (ky, kx) flattened into x) and go from L2 straight to registers; the activation window holds 16 channels and is
 * double buffered, so the loop synchronises once per window instead of once per k-step.  One 8-wave workgroup per CU owns ALL
 * couts (M == 256, or M == 128 with the K loop split between two wave groups) of a tile of nbt = 7 or 8 blocks of 32 pixels, split
 * 4 + 3 (4 + 4) so that every SIMD carries the same load: 51 200 pixels = 240 tiles of 224 on 256 CUs.  nbt = 0: the library picks.
 * M == 128 / 192 / 256, segments in multiples of 16 channels, kh, kw <= 15, < 2^22 pixels; out_vt with M != 192.  applicable: 1 = served and
 * the map gives about a workgroup per CU. */
int ppms_conv_gemm5_applicable(const ppms_conv* desc);
int ppms_conv_gemm5(const ppms_conv* desc, const ppms_conv* dev_desc, int nbt, void* stream);
/* K-sliced form of the same kernel for maps with fewer tiles than CUs (the 1/8 and 1/16 scales): nslice workgroups share each
 * tile, each sweeps its share of the activation windows and writes fp32 partial sums to the caller's workspace
 * (ppms_conv_gemm2_slice_workspace_bytes(desc, nslice)); the slice-reduce kernel then sums them in slice order and runs the fused
 * epilogue (bit-reproducible).  ppms_conv_gemm5_slices: the slice count that fills the chip in one round, 0 = not applicable. */
int ppms_conv_gemm5_slices(const ppms_conv* desc);
int ppms_conv_gemm5_sliced(const ppms_conv* desc, const ppms_conv* dev_desc, int nbt, int nslice, void* workspace, void* stream);
/* Large-map kernel on v_mfma_f32_16x16x32_bf16 (conv_gemm6.hip, round 5): ONE wave per SIMD -- a 4-wave workgroup per CU owns all couts
 * (M == 256 / 192: 64 / 48 couts x 13 pixel blocks per wave; M == 128: 64 couts x 7 or 6 blocks) of a tile of 16 rows x 13 columns = 13
 * blocks of 16 pixels: 51 200 pixels = 250 tiles on 256 CUs.  Weights in MFMA-fragment order for 16-cout x 32-channel blocks
 * (ppmstereo_amd/packing.py pack_conv6, sweep-ordered like pack_conv4), straight from L2 to registers one k32-step ahead; 32-channel
 * activation windows, column-major, double buffered by LDS-DMA through a buffer resource (the lo plane of a segment must follow its hi
 * plane inside one 4 GiB range), swept by the taps along x, along y (kh <= 5) or over all kh x kw taps; without a spatial sweep (kh = kw = 1:
 * (kt,1,1) and 1x1 convolutions) every k32-step streams its own window through a ring of three buffers.  Same descriptor and epilogues as ppms_conv_gemm5 except
 * out_vt; input segments in multiples of 32 channels.  applicable: 0 = not served, 1 = served and the 208-pixel tiles fill >= 85 % of the CU-slots of the launch's rounds,
 * 2 = served with a poor fill (a caller keeps ppms_conv_gemm5 there). */
int ppms_conv_gemm6_applicable(const ppms_conv* desc);
int ppms_conv_gemm6(const ppms_conv* desc, const ppms_conv* dev_desc, void* stream);
/* Thin GEMM for 1x1 convolutions / Linear layers (gemm1.hip): kt = kh = kw = 1, K = 128 / 192 / 256 / 384 / 512 input channels in one or two
 * 16-channel-aligned segments, M % 32 == 0, weights in the pack_gemm1 layout ([M/32][K/16][hi, lo][lane][8]: the MFMA A-operand image).
 * One workgroup = four waves that split K between them, both operands straight to registers, partial tiles summed through LDS in wave
 * order, the shared row epilogue (every kind but ADDF32; out_vt with a STORE epilogue): one memory round trip deep, no slices. */
/* 0: not served; 1: served and the faster choice (maps of <= 16 384 pixels, or <= 64 couts); 2: served, the implicit GEMM is as fast */
int ppms_gemm1_applicable(const ppms_conv* desc);
/* cb_hint: 32-cout blocks per workgroup (1, 2, 4), 0 = let the library choose from the grid size */
int ppms_gemm1(const ppms_conv* desc, const ppms_conv* dev_desc, int cb_hint, void* stream);
/* Register-streamed convolution for small maps (conv_stream.hip; the 1/8 and 1/16 scales, where ppms_conv_gemm2 needs K slices and a reduce
 * launch to fill the chip): any odd (kt, kh, kw), input channels a multiple of 64 in one or two 16-channel-aligned segments, M % 64 == 0,
 * weights in the pack_stream layout ([M/32][tap][K/16][hi, lo][lane][8], taps in natural order).  One workgroup = four waves that share the
 * 16-channel chunks of every tap of ONE 32- or 64-pixel x 64-cout tile; both operands go straight to registers through a ring of requests
 * (no LDS, no barrier in the K loop); partial tiles summed through LDS in wave order; the shared row epilogue (every kind but ADDF32, no
 * out_vt).  No workspace, no second launch, bit-reproducible.  Replaces, for the same ppms_conv descriptor, what the reference runs as one
 * cuDNN convolution (ppmtereo_update.py:254-312, 445-482, 670-678, 889-893, 910-914).
 * applicable: 0 = not served; 1 = served AND measured faster than the LDS-staged kernels with their K slices + reduce launch; 2 = served,
 * but the LDS-staged kernels (ppms_conv_gemm2 / _sliced) win -- a binding sends a convolution here only on 1.  The rating
 * (conv_stream.hip, profiles/r04_conv_stream_probe.txt): maps of <= 4 096 pixels while pixels x K x M <= 4e9 (K = taps x input channels);
 * larger maps only without spatial taps (kt > 1 or K >= 768) up to 32 768 pixels, and 64-cout convolutions up to 16 384 pixels. */
int ppms_conv_stream_applicable(const ppms_conv* desc);
/* hint: 0 = the library chooses the tile from the grid size; 1 / 2 = 32- / 64-pixel tiles.  Any other value is refused (PPMS_EINVAL). */
int ppms_conv_stream(const ppms_conv* desc, const ppms_conv* dev_desc, int hint, void* stream);
/* sizeof(ppms_sp), sizeof(ppms_epilogue), sizeof(ppms_conv) as compiled: lets a foreign-language binding check its
 * struct layout at load time */
int ppms_struct_sizes(int* sp, int* epilogue, int* conv);

/* ---------------------------------------------------------------- small ops of the update block */
/* depthwise k x k conv + residual GELU of PCBlock4_Deep_nopool_res (ppmtereo_update.py:1026-1027):
 * y = gelu(x + dw(x) + b) on an SP tensor; w: fp32 [C][k*k], b: fp32 [C]; k in {1,7}.  x, y: views of the same c <= 64 channels, c and both
 * ld multiples of 8; only the c channels of y are written.  The kernel moves 8 channels of a plane and 4 floats of the bias per load, so
 * the four plane pointers and b must be 16-byte aligned (a view of a 16-byte aligned tensor that starts at a multiple of 8 channels is): a
 * view starting at channel 4, or a bias pointer one float into its allocation, is refused with PPMS_EINVAL before any launch -- as are a
 * NULL w or b and a map with BT, H or W <= 0. */
int ppms_dwconv_gelu(ppms_sp x, ppms_sp y, const float* w, const float* b, int k, int BT, int H, int W, void* stream);
/* im2col of the 2-channel flow for convf1 (7x7, ppmtereo_update.py:452,477): patch[pixel][tap*2+c], 98 -> 128 zero padded */
int ppms_flow_patch7(const float* flow_nhwc, ppms_sp patch, int BT, int H, int W, void* stream);
/* uncertainty tail: sigmoid(w . x + b) per pixel (ppmtereo_update.py:891-892) + per-frame partial sums for the
 * QAM frame confidence (ppmstereo.py:506).  unc: fp32 [pixel]; partial: fp32 [BT][nblk], nblk = ceil(H*W/256). */
int ppms_unc_tail(ppms_sp x, const float* w, float bias, float* unc, float* partial, int BT, int HW, void* stream);

/* layout converters between the reference's NCHW fp32 tensors and SP / channel-last fp32 */
int ppms_nchw_to_sp(const float* src, ppms_sp dst, int BT, int C, int HW, void* stream);
int ppms_sp_to_nchw(ppms_sp src, float* dst, int BT, int C, int HW, void* stream);
int ppms_nchw_to_nhwc(const float* src, float* dst, int dst_ld, int BT, int C, int HW, void* stream);
int ppms_nhwc_to_nchw(const float* src, int src_ld, float* dst, int BT, int C, int HW, void* stream);
int ppms_f32_to_sp(const float* src, int src_ld, ppms_sp dst, int64_t pixels, void* stream);
int ppms_sp_to_f32(ppms_sp src, float* dst, int dst_ld, int64_t pixels, void* stream);

/* Tail of a few-output-channel conv evaluated as a 1x1 GEMM to (taps*cout) channels followed by a shifted sum:
 * out[p][c] = bias[c] + sum_tap y[p + d(tap)][tap*cout + c] (zero padded).  FlowHead3D.conv2, ppmtereo_update.py:674.
 * accum (may be NULL; fp32 [pixel][accum_ld]): accum[p][c] += out[p][c] in the same launch -- flow = flow + delta_flow, ppmstereo.py:571. */
int ppms_tap_gather_sum(const float* y, int y_ld, const float* bias, float* out, int out_ld, float* accum, int accum_ld, int cout, int kt, int kh,
                        int kw, int T, int H, int W, int t_halo, void* stream);   /* t_halo: frames of y readable beyond [0, T) (see ppms_conv) */
/* flow = flow + delta_flow (ppmstereo.py:571); flow: fp32 [pixel][2], dflow: fp32 [pixel][dflow_ld] */
int ppms_flow_add(float* flow_nhwc, const float* dflow, int dflow_ld, int64_t pixels, void* stream);
/* PPMStereo.convex_upsample, ppmstereo.py:185-197.  flow: fp32 [pixel][2]; mask: fp32 [pixel][mask_ld] (144 used);
 * out: fp32 NCHW (BT,2,4H,4W). */
int ppms_convex_upsample(const float* flow_nhwc, const float* mask, int mask_ld, float* out, int BT, int H, int W, void* stream);
/* PPMStereo.convex_upsample_3d, ppmstereo.py:199-228 (use_convex_3d=True): 27 spatio-temporal neighbours of one window of T
 * frames; mask: fp32 [pixel][mask_ld] (432 = 27 * 16 used, channel 16 k + 4 i + j, k = (kt*3 + ky)*3 + kx);
 * out: fp32 NCHW (T,2,4H,4W).  unfoldNd (absent third-party module) restated from its published semantics (zero padding). */
int ppms_convex_upsample_3d(const float* flow_nhwc, const float* mask, int mask_ld, float* out, int T, int H, int W, int t_halo, void* stream);
/* F.interpolate(mode="bilinear") on NCHW fp32, both align_corners modes (ppmstereo.py:578,580-587; utils.py:10-16);
 * out = mul * interp(src). */
int ppms_bilinear(const float* src, float* dst, int N, int C, int H, int W, int OH, int OW, int align_corners, float mul, void* stream);

/* Quantised disparity / depth / confidence output, one launch: from the 1/4-scale engine's state after its last iteration to the caller's
 * output planes -- what PPMStereo.forward_batch_test does after its last forward (ppmstereo.py:296-320: unpad, the kept frames, .abs()),
 * plus the conversion every caller of a stereo model writes behind it.
 * flow_up: fp32 (T, 2, H, W), the convex-upsampled flow; only channel 0 is read, in place (frame stride 2 H W).  unc: fp32 (T, H/4, W/4), the
 * uncertainty head's output; the kernel upsamples it 4x itself with ppms_bilinear's align_corners = 0 expression (mul = 1): the same bits.
 * Output pixel (f, y, x), f in [0, n_frames), y in [0, H0), x in [0, W0), reads source pixel (frame0 + f, y + pad_top, x + pad_left): the
 * frame range a sliding window keeps and the crop of InputPadder.unpad.  With d = |flow_up[., 0, ., .]| and u = |bilinear4(unc)|, every
 * operation below ONE fp32 operation rounded to nearest even (rint: ties to even), so that fp32 torch ops on the same inputs give the same bits:
 *   disparity plane   F32: d.   F16: d rounded to nearest even.   U16: min(65535, rint(d * disp_scale)), NaN -> 0  (KITTI: disp_scale = 256).
 *   depth plane       Z = fb / d, a correctly rounded fp32 division; fb = focal length in pixels * baseline, one fp32 product made by the caller.
 *                     The pixel is INVALID when d < min_disp or d is NaN: F32 / F16 store +inf, U16 stores 0.
 *                     Otherwise F32: Z.   F16: Z rounded to nearest even.   U16: min(65535, rint(Z * depth_scale))  (millimetres: baseline in
 *                     metres and depth_scale = 1000) -- the division and the product are rounded separately.
 *   uncertainty plane F32: u.   U8: min(255, rint(u * 255)), NaN -> 0  (u is a sigmoid output in [0, 1]).
 * A plane: device pointer to element (0, 0, 0), bytes from frame to frame and from row to row (a pitch may exceed the row: the bytes between
 * rows are not written; pointer, pitch and frame_stride multiples of the element size), its format.  ptr == NULL skips the plane.
 * `out` is HOST memory, read before the call returns.  Refused with PPMS_EINVAL before any launch: no plane; a format unknown or not listed for
 * its plane; a crop outside H x W, or H, W not multiples of 4; n_frames <= 0 or frame0 + n_frames > T; a pitch shorter than its row (or, with
 * n_frames > 1, a frame_stride shorter than a plane); a depth plane with fb <= 0, depth_scale <= 0 or a non-finite min_disp; a U16 disparity with
 * disp_scale <= 0. */
enum { PPMS_FMT_F32 = 0, PPMS_FMT_F16 = 1, PPMS_FMT_U16 = 2, PPMS_FMT_U8 = 3,
       PPMS_FMT_RGBA8 = 4, PPMS_FMT_BGRA8 = 5 };   /* 4-byte colour pixels: the colour planes below only; every plane above refuses them */
typedef struct ppms_egress_plane {
    void* ptr;                        /* element (0, 0, 0) of the output; NULL: the plane is skipped */
    int64_t frame_stride;             /* bytes from frame f to frame f + 1 */
    int64_t pitch;                    /* bytes from row to row */
    int32_t format;                   /* PPMS_FMT_* */
    int32_t reserved;                 /* 0 */
} ppms_egress_plane;
typedef struct ppms_egress {
    ppms_egress_plane disparity, depth, uncertainty;
    float disp_scale, fb, depth_scale, min_disp;
} ppms_egress;
int ppms_disparity_egress(const float* flow_up, const float* unc, int T, int H, int W, int frame0, int n_frames, int pad_left, int pad_top,
                          int H0, int W0, const ppms_egress* out, void* stream);
int ppms_egress_struct_size(void);    /* sizeof(ppms_egress) (112): lets a binding verify its layout */

/* Point-cloud output: ppms_disparity_egress with one more plane and two gates, still ONE launch -- what a caller of a stereo model does with the
 * Q matrix of its calibration behind the network (cv2.reprojectImageTo3D and a validity mask).  Arguments, sources, crop, frame range and the three
 * planes of `base` are ppms_disparity_egress's; a struct whose points.ptr is NULL and whose gates are off writes the same bits as that call.
 * With x, y = the column and row of the pixel in the cropped H0 x W0 output plane (exact fp32 integers), d and u as above, q row major,
 * every operation ONE fp32 operation rounded to nearest even, in this order:
 *   v_i  = ((q[4i] * x + q[4i+1] * y) + q[4i+2] * d) + q[4i+3]          i = 0..3
 *   X, Y, Z = v_0 / v_3, v_1 / v_3, v_2 / v_3                            correctly rounded divisions, as the depth plane's
 *   valid_d = d >= min_disp                                              (false for NaN)
 *   valid_u = max_uncertainty is +inf (gate off), or u <= max_uncertainty (false for NaN)
 *   a point is valid when valid_d and valid_u and (max_depth is +inf (gate off), or Z > 0 and Z <= max_depth)
 *   a depth pixel is valid when valid_d and valid_u and (max_depth is +inf, or fb / d <= max_depth)
 * points plane: points_components (3 or 4) elements per pixel, X, Y, Z[, w], pixel after pixel along the row: F32 the values, F16 their rounding
 * to nearest even (overflow: inf).  An invalid point carries NaN in X, Y and Z (the payload is unspecified); w = u, written for valid and invalid
 * points alike.  pitch and frame_stride are bytes as for the other planes; a row is W0 * points_components elements.  An invalid depth pixel is
 * +inf (U16: 0) as above.  The gates never touch the disparity and uncertainty planes.  q is the caller's (cv2.stereoRectify's Q for the left camera
 * with a positive disparity has the rows [1 0 0 -cx], [0 1 0 -cy], [0 0 0 f], [0 0 1/B (cx_right - cx)/B]); nothing here is compared with OpenCV.
 * Refused with PPMS_EINVAL before any launch: everything ppms_disparity_egress refuses (one shared check); no plane at all; points.format other than
 * F32 / F16; points_components other than 3 or 4 with a points plane; a points pitch shorter than W0 * points_components elements; a pitch or
 * frame_stride that is no multiple of the element; frames that overlap; a non-finite entry of q or min_disp with a points plane; a NaN max_uncertainty;
 * max_depth <= 0 or NaN; unc == NULL where a gate on u or points_components = 4 reads it; a depth plane without fb > 0; reserved != 0. */
typedef struct ppms_egress3d {
    ppms_egress base;                 /* the three planes and four constants of ppms_disparity_egress */
    ppms_egress_plane points;         /* format PPMS_FMT_F32 or PPMS_FMT_F16; ptr == NULL: no points */
    float q[16];                      /* the 4x4 reprojection matrix, row major */
    float max_uncertainty, max_depth; /* +inf: the gate is off */
    int32_t points_components;        /* 3: X Y Z.  4: X Y Z w */
    int32_t reserved;                 /* 0 */
} ppms_egress3d;
int ppms_scene_egress(const float* flow_up, const float* unc, int T, int H, int W, int frame0, int n_frames, int pad_left, int pad_top,
                      int H0, int W0, const ppms_egress3d* out, void* stream);
int ppms_egress3d_struct_size(void);  /* sizeof(ppms_egress3d) (224) */

/* Compact point cloud: the valid points only, counted, in row order -- what every consumer of the organised cloud does first
 * (pts[~pts[..., 2].isnan()]), done on the device, so that only the valid records need to cross the bus.  Arguments, sources, crop and frame
 * range are ppms_scene_egress's.  For output frame f of the launch let P[f] be the organised points plane ppms_scene_egress writes for the same
 * arguments (crop, frame range, q, min_disp, both gates, 3 or 4 components, F32 / F16) and valid[f][y][x] that call's point validity.  Then
 *   the cloud of frame f is the records of P[f] at the valid pixels, in increasing y * W0 + x, stored densely from record 0 of the frame
 *   (record k of frame f at records + f * frame_stride + k * components * element bytes): the same bits, and no record holds a NaN in X, Y, Z;
 *   counts[f] = the number of valid pixels of frame f;
 *   index[f][k] = y * W0 + x (int32) of record k, when index is not NULL (at index + f * index_frame_stride + 4 k);
 *   with capacity < counts[f] exactly the first capacity records and indices are written; counts[f] still reports the full number, so the
 *   caller sees the truncation;  records and indices at positions >= min(counts[f], capacity) are not written at all;
 *   w of 4 components is u, as in the organised plane.
 * Two launches on the stream, count and place, on one grid of (workgroups per frame, n_frames): the first writes every workgroup's number of
 * valid pixels to block_counts, the second sums the entries in front of its own, ranks its pixels and stores.  No atomics and no workgroup
 * waits for another: the order of the records is the pixels' order, the same in every run.  block_counts is workspace of
 * ppms_cloud_egress_workspace(n_frames, H0, W0) int32 entries, undefined afterwards.  `out` is HOST memory, read before the call returns.
 * Refused with PPMS_EINVAL before any launch: the geometry and the frame range ppms_disparity_egress refuses (one shared check); a null struct,
 * records, counts or flow_up; block_counts null or shorter than the workspace; unc == NULL where the max_uncertainty gate or components = 4 reads
 * it; a format other than F32 / F16; components other than 3 / 4; capacity <= 0 or above 2^31 - 1; with n_frames > 1 a frame_stride shorter than
 * capacity records or an index_frame_stride shorter than capacity indices; a pointer or stride that is no multiple of its element; a non-finite
 * entry of q or min_disp; a NaN max_uncertainty; max_depth <= 0 or NaN; reserved != 0; H0 * W0 > 2^31 - 1; n_frames > 65535. */
typedef struct ppms_cloud {
    void*    records;                 /* record 0 of frame 0 */
    int64_t  frame_stride;            /* bytes from frame to frame, >= capacity * record bytes */
    int64_t  capacity;                /* records per frame, 1 .. 2^31 - 1 */
    int32_t* index;                   /* NULL, or (n_frames, capacity) pixel indices */
    int64_t  index_frame_stride;      /* bytes */
    int32_t* counts;                  /* n_frames entries, required */
    int32_t* block_counts;            /* workspace, block_counts_len entries */
    int64_t  block_counts_len;
    float    q[16];                   /* the 4x4 reprojection matrix, row major */
    float    min_disp, max_uncertainty, max_depth;   /* +inf: gate off */
    int32_t  format;                  /* PPMS_FMT_F32 | PPMS_FMT_F16 */
    int32_t  components;              /* 3: X Y Z.  4: X Y Z w */
    int32_t  reserved;                /* 0 */
} ppms_cloud;
int     ppms_cloud_egress(const float* flow_up, const float* unc, int T, int H, int W, int frame0, int n_frames, int pad_left, int pad_top,
                          int H0, int W0, const ppms_cloud* out, void* stream);
int64_t ppms_cloud_egress_workspace(int n_frames, int H0, int W0);   /* entries block_counts needs; 0 for a geometry the call refuses */
int     ppms_cloud_struct_size(void);  /* sizeof(ppms_cloud) (152) */
/* The coloured compact cloud (XYZRGB): ppms_cloud_egress for components = 4 and PPMS_FMT_F32 with ONE change -- the fourth 32-bit word of record k
 * is the colour pixel at that record's (y, x), not the uncertainty.  `colour`: a device plane of the launch's n_frames x H0 x W0 pixels (frame f
 * of the launch, row y and column x of the crop), 4 bytes each, PPMS_FMT_RGBA8 or PPMS_FMT_BGRA8 (what ppms_video_colour_* below writes); the
 * word is copied as 32 bits, whichever of the two formats the plane names: read as a little-endian uint32 a BGRA8 pixel is 0xFFRRGGBB, the `rgb`
 * of PCL's PointXYZRGB.  The word travels as an integer from its load to its store: with alpha 255 and a third byte in 0x80..0xBF it is the
 * pattern of a signalling NaN, and no float operation may touch it.  Counts, order, indices, truncation at capacity and the bits of X, Y, Z are
 * ppms_cloud_egress's; the count launch is the same kernel, the place launch reads one aligned 32-bit word per pixel (16-byte loads where the
 * thread's run is whole and aligned).  unc is read only where the max_uncertainty gate needs it.
 * Refused with PPMS_EINVAL before any launch: everything ppms_cloud_egress refuses (one shared check; unc == NULL only with the gate on);
 * components != 4; a format other than PPMS_FMT_F32; a null colour or colour->ptr; a colour format other than the two; a colour pitch < 4 * W0;
 * with n_frames > 1 a colour frame_stride shorter than a plane; a colour pointer, pitch or frame_stride that is no multiple of 4;
 * colour->reserved != 0. */
int     ppms_cloud_egress_colour(const float* flow_up, const float* unc, int T, int H, int W, int frame0, int n_frames, int pad_left, int pad_top,
                                 int H0, int W0, const ppms_cloud* out, const ppms_egress_plane* colour, void* stream);

/* Surface normals: one unit normal per pixel of the cropped plane, from a 3 x 3 stencil (its cross: left, right, up, down) over the organised
 * points -- what a caller computes on the host from the points plane before ICP, fusion, segmentation or meshing.  One launch; arguments,
 * sources, crop and frame range are ppms_scene_egress's.  Per frame, over the CROPPED H0 x W0 plane only: a neighbour outside the crop does not
 * exist, even where the padded frame has a value there.  P(y, x) = (X, Y, Z): the fp32 organised points exactly as ppms_scene_egress defines
 * them (v_i, three divisions), whatever format a points plane or a cloud has; ok(y, x): their validity (d >= min_disp, the max_uncertainty gate,
 * the max_depth gate Z > 0 && Z <= max_depth).  Every step ONE fp32 operation rounded to nearest even, in the order written:
 *   1. neighbour N of centre C is usable iff N is inside the crop, ok(N) and ok(C), and (max_jump is +inf (gate off, not evaluated), or
 *      fabsf(Z_N - Z_C) <= max_jump * fabsf(Z_C))
 *   2. tangents.  Horizontal, L = (y, x - 1), R = (y, x + 1): both usable tx = P_R - P_L; only R: tx = P_R - P_C; only L: tx = P_C - P_L; neither:
 *      the normal is invalid.  Vertical ty likewise with U = (y - 1, x) as the minus side and D = (y + 1, x) as the plus side.
 *   3. n = ty x tx, each component two products and one subtraction:
 *      n0 = ty1 * tx2 - ty2 * tx1,  n1 = ty2 * tx0 - ty0 * tx2,  n2 = ty0 * tx1 - ty1 * tx0
 *   4. orientation towards the origin: s = (n0 * X + n1 * Y) + n2 * Z of the centre; if s > 0 then n = -n
 *   5. l = sqrt((n0 * n0 + n1 * n1) + n2 * n2), correctly rounded.  The normal is valid iff ok(C), both tangents exist, l > 0 and l is finite;
 *      a valid normal is n_i / l (correctly rounded divisions), an invalid one carries NaN in all three components (payload unspecified).
 * normals plane: 3 elements per pixel, nx, ny, nz, pixel after pixel along the row (a row: W0 * 3 elements; pitch and frame_stride in bytes):
 * F32 the values, F16 their rounding to nearest even.  The kernel computes every point of a 16 x 128 tile and its one-pixel rim once, keeps them
 * in LDS and forms the stencil from there; nobody has timed it.  `out` is HOST memory, read before the call returns.
 * Refused with PPMS_EINVAL before any launch: the geometry and the frame range ppms_disparity_egress refuses (one shared check); a null struct,
 * normals.ptr or flow_up; normals.format other than F32 / F16; a pitch shorter than the row, with n_frames > 1 a frame_stride shorter than a
 * plane, a pointer, pitch or frame_stride that is no multiple of the element; normals.reserved != 0; a non-finite entry of q or min_disp; a NaN
 * max_uncertainty; max_depth <= 0 or NaN; max_jump <= 0 or NaN; unc == NULL with the max_uncertainty gate on; reserved != 0; n_frames > 65535.
 * Not covered: larger stencils or smoothing, curvature, the right view, integer-packed normals. */
typedef struct ppms_normals {
    ppms_egress_plane normals;        /* n_frames x H0 rows of W0 * 3 elements, PPMS_FMT_F32 or PPMS_FMT_F16 */
    float q[16];                      /* the 4x4 reprojection matrix, row major */
    float min_disp, max_uncertainty, max_depth;   /* +inf: gate off (the last two) */
    float max_jump;                   /* > 0; +inf: the jump gate is off */
    int32_t reserved;                 /* 0 */
} ppms_normals;
int     ppms_normals_egress(const float* flow_up, const float* unc, int T, int H, int W, int frame0, int n_frames, int pad_left, int pad_top,
                            int H0, int W0, const ppms_normals* out, void* stream);
int     ppms_normals_struct_size(void);   /* sizeof(ppms_normals) (120) */
/* The oriented compact cloud (PCL's PointNormal / PointXYZRGBNormal): ppms_cloud_egress with the normal behind every record.  `normals`: the device
 * plane ppms_normals_egress wrote for the same arguments (n_frames x H0 x W0 x 3, frame f of the launch); the cloud's launches READ it, as the
 * coloured cloud reads the colour plane, and do not recompute the stencil.
 *   out->components = 6: records X, Y, Z, nx, ny, nz in out->format (F32: 24 bytes, F16: 12); normals->format must equal out->format; colour
 *                        must be NULL
 *   out->components = 7: records X, Y, Z, colour word, nx, ny, nz (28 bytes); out->format and normals->format PPMS_FMT_F32; colour is required
 *                        (ppms_cloud_egress_colour's plane)
 * A record is kept iff its point is valid AND its normal is valid: the first component of the normals plane is not NaN at that pixel.  Point
 * validity and the bits of X, Y, Z are ppms_cloud_egress's; the normal's words and the colour word travel as integers from their loads to their
 * stores.  counts, order, index, truncation at capacity: as ppms_cloud_egress (counts report the full number; rows past min(count, capacity) are
 * never written).  Two launches, count then place, no atomics, the same order in every run.  A workgroup takes half the pixels of
 * ppms_cloud_egress's (its staged records are up to 28 bytes), so block_counts is workspace of ppms_cloud_egress_normals_workspace entries.
 * Refused with PPMS_EINVAL before any launch: everything ppms_cloud_egress refuses (one shared check; unc == NULL only with the gate on), with
 * components other than 6 / 7 in the place of 3 / 4; a null normals or normals->ptr; a normals format other than F32 / F16 or other than
 * out->format; a normals pitch, frame_stride or alignment egress planes are refused for; normals->reserved != 0; components = 6 with a colour
 * plane; components = 7 without one, with a format other than F32, or with a colour plane ppms_cloud_egress_colour refuses. */
int     ppms_cloud_egress_normals(const float* flow_up, const float* unc, int T, int H, int W, int frame0, int n_frames, int pad_left, int pad_top,
                                  int H0, int W0, const ppms_cloud* out, const ppms_egress_plane* normals, const ppms_egress_plane* colour, void* stream);
int64_t ppms_cloud_egress_normals_workspace(int n_frames, int H0, int W0);   /* entries block_counts needs; 0 for a geometry the call refuses */

/* Scale-to-scale hand-over of the cascade without leaving the SP format (ppmstereo.py:726-732, 763-767): per frame,
 * dst = a * dst + b * interp(src), interp = F.interpolate(mode="bilinear", align_corners=True) from HxW to OHxOW.
 * src, dst: SP views with the same channel count (multiple of 8). */
int ppms_sp_resize_blend(ppms_sp src, ppms_sp dst, int N, int H, int W, int OH, int OW, float a, float b, void* stream);

/* Pre-loop glue of PPMStereo.forward (ppmstereo.py:620-682), NCHW fp32: avg_pool2d(k, stride k) of `planes` HxW planes;
 * out = a x + b y[i mod period] (plain or frame-broadcast axpby); net = tanh((f[:, :128] + c[:, :128]) / 2),
 * inp = relu((f[:, 128:] + c[:, 128:]) / 2) for f, c of shape (N, 256, HW). */
int ppms_avgpool(const float* src, float* dst, int planes, int H, int W, int k, void* stream);
int ppms_axpby(const float* x, const float* y, float* out, float a, float b, int64_t period, int64_t n, void* stream);
int ppms_ctx_mix(const float* fmap, const float* ctx, float* net, float* inp, int N, int HW, void* stream);

/* ---------------------------------------------------------------- feature encoder (fnet) pieces
 * BasicEncoder(output_dim=256, norm_fn="instance"), extractor.py:302-423.  Its convolutions run on
 * ppms_conv_gemm2 / ppms_conv_gemm5; the stride-2 layers (extractor.py:306-308, 341-343, 366) as stride-1 convolutions over a
 * 2x2 space-to-depth copy of their input: dst[(n, i, j)][(2 dy + dx) * C + c] = src[(n, 2 i + dy, 2 j + dx)][c].
 * ppms_img_s2d: src = the NCHW fp32 image batch (N, C, H, W) handed to the encoders (extractor.py:400-405, convnext.py:257),
 * factor k (phase = k dy + dx); channels >= k*k*C of dst are zeroed.  ppms_sp_s2d: src, dst split-plane views, factor 2,
 * dst.c == 4 * src.c.  H, W multiples of the factor. */
int ppms_img_s2d(const float* img_nchw, ppms_sp dst, int N, int C, int H, int W, int k, void* stream);   /* k = 2 (fnet), 4 (cnet stem) */
int ppms_sp_s2d(ppms_sp src, ppms_sp dst, int N, int H, int W, void* stream);
/* uint8 video -> both encoders' first-layer operands, one launch: for byte frames (3, H0, W0) in CHW order -- `left` / `right` point to
 * frame 0 of each view, consecutive frames of a view are `frame_stride` bytes apart (a (T, 2, 3, H0, W0) window: right = left + 3 H0 W0,
 * stride 6 H0 W0; two (N, 3, H0, W0) tensors: stride 3 H0 W0) -- it writes what normalising with lut[byte] (device fp32 [256]), replicate
 * padding to H x W (pad_left columns / pad_top rows in front, the rest behind; H, W multiples of 4), torch.cat([left, right]) and
 * ppms_img_s2d give: dst_fnet = the k = 2 operand of the 2 N images (the N left frames first), dst_cnet = the k = 4 operand of the N left
 * frames.  Channel order, zeroed channels >= 3 k k and the alignment contract are ppms_img_s2d's.  hi == NULL skips a destination. */
int ppms_video_ingest_u8(const uint8_t* left, const uint8_t* right, int64_t frame_stride, int N, int H0, int W0, int pad_left, int pad_top, int H, int W,
                         const float* lut, ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream);
/* The same two operands from decoded YUV 4:2:0 frames (NV12, I420 / yuv420p; 8 bits), one launch: a view describes one eye's N frames as the
 * decoder left them -- a pitched Y plane of H0 x W0 bytes and chroma planes of ceil(H0/2) x ceil(W0/2) samples, planar (step_c = 1) or interleaved
 * (step_c = 2, v == u + 1 for NV12); both views of a side-by-side or top-and-bottom packed frame are two views into one surface.  Luma pixel
 * (y, x) -- after the replicate-padding clamp -- takes chroma sample (y >> 1, x >> 1) (nearest; odd H0, W0 are legal), and its RGB bytes are,
 * in integers (>> is the arithmetic shift, r = 1 << (shift - 1), d = Y - y_off, e = U - 128, f = V - 128):
 *   R = clamp((cy d + crv f + r) >> shift, 0, 255), G = clamp((cy d - cgu e - cgv f + r) >> shift, 0, 255), B = clamp((cy d + cbu e + r) >> shift, 0, 255)
 * (shift in [8, 20], y_off in [0, 255], coefficients in [0, 4 << shift): no sum leaves 32 bits).  From those bytes on -- lut, pads, H x W,
 * destinations, hi == NULL -- the call is ppms_video_ingest_u8 on channel order R, G, B.  The three structs are HOST memory, read before the
 * call returns; every pointer inside a view is a device pointer.  10- and 12-bit surfaces (P010 ...) and 4:2:2 / 4:4:4: ppms_video_ingest_yuv below. */
typedef struct ppms_yuv_view {        /* one view's frames, as the decoder left them */
    const uint8_t *y, *u, *v;         /* sample (0,0) of frame 0; interleaved UV: v == u + 1 */
    int64_t frame_stride_y, frame_stride_c;   /* bytes from frame n to frame n + 1 */
    int32_t pitch_y, pitch_c;         /* bytes from row to row */
    int32_t step_c;                   /* bytes from chroma sample to chroma sample: 1 (planar) or 2 (interleaved) */
    int32_t reserved;                 /* 0 */
} ppms_yuv_view;
typedef struct ppms_yuv_matrix {      /* fixed-point YCbCr -> RGB, see above */
    int32_t y_off, cy, crv, cgu, cgv, cbu, shift, reserved;
} ppms_yuv_matrix;
int ppms_video_ingest_yuv420(const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m,
                             int N, int H0, int W0, int pad_left, int pad_top, int H, int W,
                             const float* lut, ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream);
int ppms_yuv_struct_sizes(int* view, int* matrix);   /* sizeof of the two structs above (56, 32): lets a binding verify its layout */
/* Both calls above on the frames of an UNRECTIFIED rig, one launch: the undistort + rectify (+ resize) remap every caller runs between the
 * decoder and a stereo model happens where the byte is fetched.  H0 x W0 is now the RECTIFIED frame; the source frames are hs x ws.  One view's
 * map covers the rectified frame and holds, for rectified pixel (y, x) at element y * pitch + x,
 *   xy:   int16 (x0, y0), interleaved, x first -- the integer part of the source coordinate;
 *   frac: a 16-bit word, fx = frac & 31, fy = (frac >> 5) & 31 -- its fraction in 1/32 pixel; bits 10 and up must be 0, and the kernel masks them.
 * (The layout OpenCV's convertMaps(..., CV_16SC2) documents for its fixed-point maps; nothing here has been compared with OpenCV.)
 * The taps are source pixels (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1) -- coordinates in 32-bit arithmetic -- with the weights
 *   w00 = (32 - fx)(32 - fy),  w01 = fx (32 - fy),  w10 = (32 - fx) fy,  w11 = fx fy          (their sum is 1024)
 * and, for each of R, G, B,   out = (w00 p00 + w01 p01 + w10 p10 + w11 p11 + 512) >> 10,   which lies in [0, 255] without a clamp; a map
 * whose frac is 0 everywhere copies bytes.  border = 0 (replicate): every tap coordinate is clamped into the source frame; border = 1
 * (constant): a tap outside the frame contributes `fill` (one byte for R, G and B).  In both modes every load address is clamped into the
 * frame first, whatever the map holds: a nonsense map gives nonsense pixels, never a read outside the surface.  For YUV sources a tap is
 * the RGB byte of that source pixel -- the conversion above, with the pixel's nearest chroma sample -- and the blend happens in RGB: the
 * result is by definition the remap of the converted frames.  From the rectified bytes on (lut, pads, H x W, destinations) the calls are
 * ppms_video_ingest_u8: the same bits as rectifying first and calling it.  The map structs are HOST memory, read before the call returns;
 * xy (4-byte aligned) and frac (2-byte aligned) are device pointers to at least (H0 - 1) * pitch + W0 elements, shared by all N frames of
 * the view.  _u8_remap: dense planar RGB source frames (3, hs, ws), frame_stride >= 3 hs ws.  _yuv420_remap: the views are checked as
 * ppms_video_ingest_yuv420 checks them, against hs x ws.  Refused with PPMS_EINVAL before any launch: a null map or a null pointer in one,
 * pitch < W0, hs or ws outside [1, 32768], the two maps' hs / ws differing, border not 0 or 1, fill outside [0, 255], reserved != 0, a
 * misaligned pointer.  Not covered: interpolation other than bilinear, computing maps from calibration data. */
typedef struct ppms_remap_view {      /* one view's rectification map */
    const int16_t* xy;                /* (x0, y0) of rectified pixel (0, 0); device pointer */
    const uint16_t* frac;             /* fx | fy << 5 of rectified pixel (0, 0); device pointer */
    int32_t pitch;                    /* map pixels from row to row, >= W0 */
    int32_t hs, ws;                   /* source frame size, 1..32768 */
    int32_t border, fill, reserved;   /* 0 = replicate, 1 = constant; the constant's byte; 0 */
} ppms_remap_view;
int ppms_video_ingest_u8_remap(const uint8_t* left, const uint8_t* right, int64_t frame_stride, const ppms_remap_view* lmap, const ppms_remap_view* rmap,
                               int N, int H0, int W0, int pad_left, int pad_top, int H, int W,
                               const float* lut, ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream);
int ppms_video_ingest_yuv420_remap(const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m,
                                   const ppms_remap_view* lmap, const ppms_remap_view* rmap,
                                   int N, int H0, int W0, int pad_left, int pad_top, int H, int W,
                                   const float* lut, ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream);
int ppms_remap_struct_size(int* view);               /* sizeof(ppms_remap_view) (40): lets a binding verify its layout */
/* ppms_video_ingest_yuv420 and its _remap twin for the other surfaces decoders deliver: 10- and 12-bit samples in little-endian 16-bit words
 * (P010 / P012 / P210: bits at the top; yuv420p10le / yuv422p10le / yuv444p12le ...: bits at the bottom) and 4:2:2 / 4:4:4 chroma at any depth (NV16,
 * yuv422p, yuv444p).  `fmt` (HOST memory, read before the call returns) says how to read the views; the views and the matrix are the structs above.
 *   Samples and strides.  A sample is (word >> lsb) & ((1 << depth) - 1): with lsb = 16 - depth the low bits of the word are dropped whatever they
 * hold, with lsb = 0 the high bits are masked.  Every stride of a view stays in BYTES; step_c = sample_bytes (planar) or 2 * sample_bytes
 * (interleaved, v == u + sample_bytes); with sample_bytes = 2 every pointer, pitch and frame stride must be even.  The chroma planes hold
 * ceil(H0 / 2^sub_y) x ceil(W0 / 2^sub_x) samples, and luma pixel (y, x) -- after the replicate-padding clamp -- takes chroma sample
 * (y >> sub_y, x >> sub_x) (nearest; odd H0, W0 are legal).
 *   Conversion.  The integer formula of ppms_video_ingest_yuv420 with e = U - (1 << (depth - 1)), f = V - (1 << (depth - 1)) and the results clamped
 * to [0, 2^depth - 1]: RGB LEVELS of `depth` bits.  y_off in [0, 2^depth), shift in [8, 26 - depth], coefficients in [0, 4 << shift): no sum leaves
 * 32 bits (three terms below 4 * 2^shift * 2^depth <= 2^28 each, plus the rounding term, stay below 2^31).
 *   Level table.  lut is a device fp32 array of 1 << depth entries, indexed by the RGB level; from the levels on -- lut, pads, H x W, destinations,
 * hi == NULL -- the call is ppms_video_ingest_u8.  With fmt = {1, 8, 0, 1, 1} it writes ppms_video_ingest_yuv420's bits.
 *   _remap.  The remap contract above on the source's levels: a tap is the RGB level of that source pixel, the blend (sum w p + 512) >> 10 lies in
 * [0, 2^depth - 1] without a clamp, and `fill` is a level in [0, 2^depth - 1].
 *   Refused with PPMS_EINVAL before any launch: whatever ppms_video_ingest_yuv420 (_remap) refuses, restated for these samples; sample_bytes not 1
 * or 2; a depth that does not go with it (8 with 1; 10 or 12 with 2); lsb not 0 or 16 - depth; (sub_x, sub_y) not (1,1), (1,0) or (0,0) -- (0,1)
 * included; non-zero reserved; an odd pointer or stride with 16-bit samples; a pitch or frame stride too small for the sample size and the
 * subsampling; shift, y_off or fill outside the bounds above.
 * Not covered: interpolated chroma siting, 16-bit depth, BT.2020 and HDR transfer functions, planar high-depth RGB.  (Packed YUYV / Y210 / v210:
 * ppms_video_ingest_yuv_packed below; interleaved RGB of 8, 10 or 12 bits: ppms_video_ingest_rgb_packed.) */
typedef struct ppms_yuv_format {
    int32_t sample_bytes;             /* 1, or 2 (little-endian 16-bit words) */
    int32_t depth;                    /* 8 with sample_bytes 1; 10 or 12 with sample_bytes 2 */
    int32_t lsb;                      /* bit of the word that holds the sample's lowest bit: 0 (yuv420p10le ...) or 16 - depth (P010, P012, P210 ...); 0 for bytes */
    int32_t sub_x, sub_y;             /* log2 chroma subsampling: (1,1) 4:2:0, (1,0) 4:2:2, (0,0) 4:4:4 */
    int32_t reserved[3];              /* 0 */
} ppms_yuv_format;
int ppms_video_ingest_yuv(const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, const ppms_yuv_format* fmt,
                          int N, int H0, int W0, int pad_left, int pad_top, int H, int W,
                          const float* lut, ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream);
int ppms_video_ingest_yuv_remap(const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, const ppms_yuv_format* fmt,
                                const ppms_remap_view* lmap, const ppms_remap_view* rmap,
                                int N, int H0, int W0, int pad_left, int pad_top, int H, int W,
                                const float* lut, ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream);
int ppms_yuv_format_struct_size(int* fmt);           /* sizeof(ppms_yuv_format) (32): lets a binding verify its layout */
/* The same two operands from the RAW frames of a sensor that has no decoder behind it (machine-vision heads: GigE / USB3-Vision, MIPI), one launch:
 * a Bayer colour-filter mosaic (BayerRG8, BayerGB10, BayerRG12 ...) or a monochrome plane (Mono8 / Mono10 / Mono12), one sample per pixel.  A view
 * describes one eye's N frames as the camera driver left them: one pitched plane of H0 x W0 samples; both views of a side-by-side or top-and-bottom
 * packed frame are two views into one surface.  `fmt` (HOST memory, read before the call returns) is shared by both views; every pointer inside a
 * view is a device pointer.
 *   Samples and strides.  ppms_yuv_format's: sample_bytes = 1 with depth 8, or 2 (little-endian 16-bit words) with depth 10 or 12; lsb = 0 or
 * 16 - depth; a sample is (word >> lsb) & ((1 << depth) - 1).  pitch and frame_stride are in BYTES, and even -- as the pointer -- for 16-bit samples.
 *   Mosaic.  pattern 0 = RGGB, 1 = BGGR, 2 = GRBG, 3 = GBRG, 4 = MONO: the name spells the 2 x 2 tile at the frame's origin in row-major order, and
 * the colour of source pixel (y, x) is tile[(y & 1) * 2 + (x & 1)].  Let s(y, x) be the sample at source coordinate (y, x) of a frame of hs x ws
 * (H0 x W0 without a map).  A NEIGHBOUR coordinate outside the frame is reflected without repeating the edge, t < 0 -> -t, t > n - 1 ->
 * 2 (n - 1) - t, which keeps the colour-filter parity for every frame size (hence hs, ws >= 2 for the four colour patterns).  For a site of
 * colour k and the wanted channel c:
 *   c == k:                                   v = s(y, x)
 *   k in {R, B}, c == G:                      v = (s(y-1, x) + s(y+1, x) + s(y, x-1) + s(y, x+1) + 2) >> 2
 *   k in {R, B}, c the other of R / B:        v = (s(y-1, x-1) + s(y-1, x+1) + s(y+1, x-1) + s(y+1, x+1) + 2) >> 2
 *   k == G, c in {R, B}:                      v = (s(y, x-1) + s(y, x+1) + 1) >> 1 if this row's horizontal neighbours carry c,
 *                                             v = (s(y-1, x) + s(y+1, x) + 1) >> 1 otherwise
 *   MONO:                                     v = s(y, x) for all three channels
 * (bilinear demosaicing; nothing here has been compared with OpenCV's demosaic).
 *   Black level and white balance.  The RGB LEVEL of channel c is, in integers (>> is the arithmetic shift, as in the YUV formula),
 *   level = clamp(((v - black) * gain[c] + (1 << (shift - 1))) >> shift, 0, 2^depth - 1)
 * with black in [0, 2^depth), shift in [4, 14] and gain[0..2] (R, G, B) in [0, 16 << shift): no sum leaves 32 bits (2^12 * 2^18 + 2^13 < 2^31).
 *   Level table.  lut is a device fp32 array of 1 << depth entries, indexed by the RGB level; from the levels on -- lut, pads, H x W, destinations,
 * hi == NULL -- the call is ppms_video_ingest_yuv.  The table is the caller's: a tone curve (gamma / sRGB encoding of linear sensor data) is
 * another table and costs nothing.
 *   _remap.  The remap contract above on these levels: a tap is the RGB level of that source pixel, demosaiced in the SOURCE frame (its neighbours
 * reflected at the source frame's edges); the blend (sum w p + 512) >> 10 lies in [0, 2^depth - 1] without a clamp, and `fill` is a level in
 * [0, 2^depth - 1].  Every load address comes from a coordinate clamped or reflected into the frame, whatever the map holds.
 *   Refused with PPMS_EINVAL before any launch: a null pointer; non-zero reserved; sample_bytes not 1 or 2; a depth that does not go with it; lsb
 * not 0 or 16 - depth; pattern outside 0..4; black, a gain or shift outside the bounds above; an odd pointer, pitch or frame stride with 16-bit
 * samples; a pitch shorter than a row; with N > 1 a frame_stride shorter than a frame; a frame smaller than 2 x 2 with a colour pattern; what
 * ppms_video_ingest_u8 refuses about sizes, pads and destinations; for _remap, whatever the _remap calls above refuse.
 * Not covered: 14- and 16-bit sensors (the level table would not fit LDS), demosaicing better than bilinear, colour-correction matrices, lens
 * shading and defect pixels, patterns that differ between the two views.  (Packed 10p / 12p transport formats: ppms_video_ingest_raw_packed below.) */
typedef struct ppms_raw_view {        /* one view's frames, as the camera driver left them */
    const uint8_t* data;              /* sample (0,0) of frame 0 */
    int64_t frame_stride;             /* bytes from frame n to frame n + 1 */
    int32_t pitch;                    /* bytes from row to row */
    int32_t reserved;                 /* 0 */
} ppms_raw_view;
typedef struct ppms_raw_format {
    int32_t sample_bytes;             /* 1, or 2 (little-endian 16-bit words) */
    int32_t depth;                    /* 8 with sample_bytes 1; 10 or 12 with sample_bytes 2 */
    int32_t lsb;                      /* bit of the word that holds the sample's lowest bit: 0 or 16 - depth; 0 for bytes */
    int32_t pattern;                  /* 0 RGGB, 1 BGGR, 2 GRBG, 3 GBRG, 4 MONO */
    int32_t black;                    /* black level, [0, 2^depth) */
    int32_t gain[3];                  /* white balance for R, G, B times 2^shift, [0, 16 << shift) */
    int32_t shift;                    /* [4, 14] */
    int32_t reserved[3];              /* 0 */
} ppms_raw_format;
int ppms_video_ingest_raw(const ppms_raw_view* left, const ppms_raw_view* right, const ppms_raw_format* fmt,
                          int N, int H0, int W0, int pad_left, int pad_top, int H, int W,
                          const float* lut, ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream);
int ppms_video_ingest_raw_remap(const ppms_raw_view* left, const ppms_raw_view* right, const ppms_raw_format* fmt,
                                const ppms_remap_view* lmap, const ppms_remap_view* rmap,
                                int N, int H0, int W0, int pad_left, int pad_top, int H, int W,
                                const float* lut, ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream);
int ppms_raw_struct_sizes(int* view, int* format);   /* sizeof of the two structs above (24, 48): lets a binding verify its layout */
/* ppms_video_ingest_yuv and ppms_video_ingest_raw (and their _remap twins) for the PACKED formats cameras and capture cards put on the wire, one
 * launch, no unpacked intermediate: YUYV / UYVY / YVYU / VYUY (UVC cameras), Y210 / Y212, v210 (SDI capture), MIPI CSI-2 RAW10 / RAW12 (V4L2
 * SRGGB10P ...) and GenICam PFNC Mono10p / BayerRG12p ....  A packed format is another way of fetching sample (y, x): each call below is DEFINED by
 * the unpacked call on the frames that hold the same samples, and writes its bits.
 *   The view.  One pitched surface per view: row y of frame n starts at data + n * frame_stride + y * pitch (BYTES).  Column x of the view is
 * surface column p = x + x0: the right half of a side-by-side frame is the same surface with another x0, which may lie in the middle of a v210 or
 * RAW10 group.  x0 must be even for YUV (a chroma pair may not be split) and may be any value >= 0 for raw (the pattern is that of the view's own
 * pixel (0, 0)); x0 + ws <= 65536.  The views and formats are HOST memory, read before the call returns; `data` is a device pointer.
 *   Packed 4:2:2 YUV.  A row is a stream of components.  For pixel p and its pair j = p >> 1 the component indices are Y = 2 p + a, U = 4 j + b,
 * V = 4 j + c with (a, b, c) = (0, 1, 3) for order 0 (yuyv), (1, 0, 2) for 1 (uyvy), (0, 3, 1) for 2 (yvyu), (1, 2, 0) for 3 (vyuy): chroma comes
 * from the pixel's own pair (nearest).  `container` says where component i lies:
 *   0   byte i of the row; depth 8 (YUY2 / YUYV, UYVY, YVYU, VYUY);
 *   1   little-endian 16-bit word i, the sample (word >> lsb) & ((1 << depth) - 1); depth 10 or 12, lsb = 16 - depth (Y210 / Y212: bits at the top, the
 *       low bits dropped whatever they hold) or 0 (bits at the bottom, the high bits masked); pointer, pitch and frame stride even;
 *   2   v210: bits [10 (i % 3), 10 (i % 3) + 10) of little-endian 32-bit word i / 3 (bits 30, 31 are ignored); depth 10, order uyvy only, lsb 0;
 *       pointer, pitch and frame stride multiples of 4.  A 16-byte group of four words therefore holds, lowest bits first,
 *           Cb0 Y0 Cr0 | Y1 Cb1 Y2 | Cr1 Y3 Cb2 | Y4 Cr2 Y5
 *       -- six pixels.  (This layout is the definition here; nothing has been compared with ffmpeg or a capture card.)
 * A row of P = x0 + ws columns holds row_bytes = 4 ceil(P / 2) (bytes), 8 ceil(P / 2) (words) or 16 ceil(P / 6) (v210): the last pair or group must
 * be whole in memory, since its chroma is read.  From the three `depth`-bit samples on -- the matrix and its bounds, the clamp, lut of 1 << depth
 * entries, pads, destinations -- the call is ppms_video_ingest_yuv with sub_x = 1, sub_y = 0 on the planar surface that holds the same samples.
 *   Packed raw.  ppms_raw_format without sample_bytes and lsb; depth 10 or 12.  Sample s(y, p) of a row of bytes:
 *   packing 0 (MIPI CSI-2; V4L2 *10P, *12P):  RAW10: g = p >> 2, k = p & 3, s = row[5 g + k] << 2 | (row[5 g + 4] >> 2 k) & 3;
 *                                             RAW12: g = p >> 1, k = p & 1, s = row[3 g + k] << 4 | (row[3 g + 2] >> 4 k) & 15;
 *   packing 1 (GenICam PFNC 10p / 12p, an lsb-first bit stream):  bit = p * depth, o = bit >> 3,
 *                                             s = ((row[o] | row[o + 1] << 8) >> (bit & 7)) & ((1 << depth) - 1)
 * (both bytes hold bits of the pixel itself: the last pixel of a row reads nothing behind the row).  row_bytes = 5 ceil(P / 4), 3 ceil(P / 2) or
 * ceil(P depth / 8).  From s on -- reflected neighbours, bilinear demosaic or mono, black level and gains, the caller's table, pads, destinations --
 * the call is ppms_video_ingest_raw on the unpacked 16-bit, lsb-aligned frames.  (Nothing has been compared with a sensor or a GenICam producer.)
 *   _remap.  The remap contract above on these levels, as for the unpacked calls; every load address comes from a coordinate clamped or reflected
 * into the frame, and with the pitch check below no load leaves [row, row + row_bytes).
 *   Refused with PPMS_EINVAL before any launch: a null pointer; non-zero reserved; container, order, packing or depth out of range or not going
 * together (v210 with anything but depth 10 and uyvy; container 0 with anything but depth 8); lsb not 0 or 16 - depth (and not 0 outside container
 * 1); x0 < 0, x0 odd for YUV, x0 + ws > 65536; an odd pointer or stride with container 1, one that is no multiple of 4 with v210; pitch <
 * row_bytes(x0 + ws); with N > 1 a frame_stride < (hs - 1) * pitch + row_bytes; a colour pattern on a frame smaller than 2 x 2; shift in [8, 26 -
 * depth], y_off and the coefficients as ppms_video_ingest_yuv bounds them; pattern, black, shift and gains as ppms_video_ingest_raw bounds them;
 * what ppms_video_ingest_u8 refuses about sizes, pads and destinations; for _remap, whatever the _remap calls above refuse.
 * Not covered: Y216 and other 16-bit depths, 14-bit packed raw, 4:4:4 packed (v410, Y410, AYUV), big-endian containers, interpolated
 * chroma siting, patterns or layouts that differ between the two views. */
typedef struct ppms_packed_view {     /* one view's frames inside a packed surface */
    const uint8_t* data;              /* column 0 of row 0 of frame 0 of the SURFACE */
    int64_t frame_stride;             /* bytes from frame n to frame n + 1 */
    int32_t pitch;                    /* bytes from row to row */
    int32_t x0;                       /* surface column of the view's column 0 */
} ppms_packed_view;
typedef struct ppms_yuv_packed_format {
    int32_t container;                /* 0 bytes, 1 little-endian 16-bit words, 2 v210 */
    int32_t depth;                    /* 8 with container 0; 10 or 12 with 1; 10 with 2 */
    int32_t lsb;                      /* container 1: 0 or 16 - depth (Y210, Y212); 0 otherwise */
    int32_t order;                    /* 0 yuyv, 1 uyvy, 2 yvyu, 3 vyuy */
    int32_t reserved[4];              /* 0 */
} ppms_yuv_packed_format;
typedef struct ppms_raw_packed_format {
    int32_t packing;                  /* 0 MIPI CSI-2, 1 PFNC lsb-first */
    int32_t depth;                    /* 10 or 12 */
    int32_t pattern;                  /* 0 RGGB, 1 BGGR, 2 GRBG, 3 GBRG, 4 MONO */
    int32_t black;                    /* black level, [0, 2^depth) */
    int32_t gain[3];                  /* white balance for R, G, B times 2^shift, [0, 16 << shift) */
    int32_t shift;                    /* [4, 14] */
    int32_t reserved[4];              /* 0 */
} ppms_raw_packed_format;
int ppms_video_ingest_yuv_packed(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_yuv_matrix* m, const ppms_yuv_packed_format* fmt,
                                 int N, int H0, int W0, int pad_left, int pad_top, int H, int W,
                                 const float* lut, ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream);
int ppms_video_ingest_yuv_packed_remap(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_yuv_matrix* m, const ppms_yuv_packed_format* fmt,
                                       const ppms_remap_view* lmap, const ppms_remap_view* rmap,
                                       int N, int H0, int W0, int pad_left, int pad_top, int H, int W,
                                       const float* lut, ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream);
int ppms_video_ingest_raw_packed(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_raw_packed_format* fmt,
                                 int N, int H0, int W0, int pad_left, int pad_top, int H, int W,
                                 const float* lut, ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream);
int ppms_video_ingest_raw_packed_remap(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_raw_packed_format* fmt,
                                       const ppms_remap_view* lmap, const ppms_remap_view* rmap,
                                       int N, int H0, int W0, int pad_left, int pad_top, int H, int W,
                                       const float* lut, ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream);
int ppms_packed_struct_sizes(int* view, int* yuv_format, int* raw_format);   /* sizeof of the three structs above (24, 32, 48): lets a binding verify its layout */
/* Interleaved RGB, (H, W, C) with the channels adjacent -- what cv2.VideoCapture / imread, PIL and numpy, GStreamer video/x-raw BGR, ROS bgr8 / rgba8,
 * DXGI / DRM capture and ffmpeg rgb24 / bgr0 / rgb48le / x2rgb10le hand over -- read where it lies: one launch, no planar intermediate.  The view is the
 * ppms_packed_view above (one pitched surface per view, column x of the view is surface column p = x + x0); x0 may be any value >= 0, since there is
 * no chroma pair to split; x0 + ws <= 65536.  `fmt` (HOST memory, read before the call returns) is shared by both views.
 *   How a level is read.  A pixel is `step` components; channel c (0 R, 1 G, 2 B) is component step * p + offset[c] of the row:
 *   container 0   byte i of the row; depth 8; step 3 (rgb24, bgr24) or 4 (rgba, bgra, argb, abgr and their x forms);
 *   container 1   little-endian 16-bit word i, the sample (word >> lsb) & ((1 << depth) - 1); depth 10 or 12, lsb = 16 - depth (bits at the top, the low
 *                 bits dropped whatever they hold) or 0 (bits at the bottom, the high bits masked); step 3 (rgb48, bgr48) or 4 (rgba64, bgra64);
 *                 pointer, pitch and frame stride even;
 *   container 2   one little-endian 32-bit word per pixel (step 1), channel c in field offset[c]: bits [10 f, 10 f + 10) of word p; bits 30 and 31 are
 *                 ignored; depth 10, lsb 0; pointer, pitch and frame stride multiples of 4.  offset = (2, 1, 0) puts R in bits 29..20, G in 19..10, B in
 *                 9..0: ffmpeg's x2rgb10le and DRM's XRGB2101010 as those projects document them; offset = (0, 1, 2) puts R in bits 9..0: DXGI's
 *                 R10G10B10A2 and ffmpeg's x2bgr10le likewise.  (The layouts are restated from that documentation: nothing has been compared with
 *                 ffmpeg, a compositor or a capture API.)
 * The component that no offset names -- the fourth of a step-4 pixel: alpha or padding -- is never loaded.  A row of P = x0 + ws columns holds
 * row_bytes = step * P (bytes), 2 * step * P (words) or 4 * P (container 2).  The sample IS the level: from it on -- lut of 1 << depth entries, replicate
 * padding, destinations -- the call is ppms_video_ingest_u8 on the planar frames that hold the same levels, with the table of that depth; at depth 8 it
 * writes ppms_video_ingest_u8's bits.
 *   _remap.  The remap contract above on these levels with fill in [0, 2^depth - 1]; every load address comes from a coordinate clamped into the frame,
 * and with the pitch check below no load leaves [row, row + row_bytes).
 *   Refused with PPMS_EINVAL before any launch: a null pointer; non-zero reserved; container, depth, lsb or step out of range or not going together
 * (container 0 with anything but depth 8, 2 with anything but depth 10, lsb 0 and step 1; lsb not 0 or 16 - depth, and not 0 outside container 1; step
 * not 3 or 4 with containers 0 and 1); an offset outside [0, step) (container 2: outside {0, 1, 2}) or two equal offsets; x0 < 0, x0 + ws > 65536; an odd
 * pointer or stride with container 1, one that is no multiple of 4 with container 2; pitch < row_bytes(x0 + ws); with N > 1 a frame_stride <
 * (hs - 1) * pitch + row_bytes; what ppms_video_ingest_u8 refuses about sizes, pads and destinations; for _remap, whatever the _remap calls above refuse.
 * Not covered: 16-bit depth (the level table would not fit LDS), planar high-depth RGB (gbrp10le), big-endian words, RGB565, premultiplied or
 * meaningful alpha, float / half RGB surfaces, layouts that differ between the two views. */
typedef struct ppms_rgb_packed_format {
    int32_t container;                /* 0 bytes, 1 little-endian 16-bit words, 2 one little-endian 32-bit word of three 10-bit fields */
    int32_t depth;                    /* 8 with container 0; 10 or 12 with 1; 10 with 2 */
    int32_t lsb;                      /* container 1: 0 or 16 - depth; 0 otherwise */
    int32_t step;                     /* components per pixel: 3 or 4 (containers 0, 1); 1 (container 2) */
    int32_t offset[3];                /* where R, G, B lie inside the pixel: component index in [0, step), distinct (containers 0, 1);
                                         field index in {0, 1, 2}, distinct: bits [10 f, 10 f + 10) of the word (container 2; bits 30, 31 ignored) */
    int32_t reserved;                 /* 0 */
} ppms_rgb_packed_format;
int ppms_video_ingest_rgb_packed(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_rgb_packed_format* fmt,
                                 int N, int H0, int W0, int pad_left, int pad_top, int H, int W,
                                 const float* lut, ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream);
int ppms_video_ingest_rgb_packed_remap(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_rgb_packed_format* fmt,
                                       const ppms_remap_view* lmap, const ppms_remap_view* rmap,
                                       int N, int H0, int W0, int pad_left, int pad_top, int H, int W,
                                       const float* lut, ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream);
int ppms_rgb_packed_struct_size(int* fmt);   /* sizeof of ppms_rgb_packed_format (32): lets a binding verify its layout */
/* Colour out: the LEFT view as the network saw it -- converted, demosaiced, white-balanced, tone-mapped, rectified -- as 4-byte pixels registered
 * to the egress planes, one launch.  One entry point per ingest door above, with that door's head arguments (and maps), the same sources and the
 * same checks of them; the right view's pointers and structs stay in the signature and are checked, and never read by the kernel.
 * Output pixel (f, y, x), f in [0, n_frames), y in [0, h0), x in [0, w0), is the pixel (clamp(y + y0, 0, H0 - 1), clamp(x + x0, 0, W0 - 1)) of left
 * frame frame0 + f of the H0 x W0 frame (the rectified frame for _remap): x0 = crop_left - pad_left, y0 = crop_top - pad_top of an egress crop inside
 * the padded frame, so a crop that reaches into the padding sees the replicate padding the network saw; x0, y0 may be negative or reach past the frame.
 * Each of the pixel's three levels (the door's own R, G, B of `depth` bits) is looked up in `table`, device uint8 [2^depth] (256 for the u8 and
 * yuv420 doors): the byte the level stands for, built by the caller (clamp(rint(float value), 0, 255), ties to even; a raw format's tone curve goes
 * here).  The pixel's four bytes in memory are R, G, B, 255 (PPMS_FMT_RGBA8) or B, G, R, 255 (PPMS_FMT_BGRA8).  `out`: HOST struct, a device plane of
 * n_frames x h0 x w0 pixels with byte strides (bytes between the rows of a pitched plane are not written).
 * Refused with PPMS_EINVAL before any launch: everything the door's ingest twin refuses about sources, formats and maps; a null table, out or
 * out->ptr; a format other than the two; a pitch < 4 * w0; with n_frames > 1 a frame_stride shorter than a plane (frames that overlap); a pointer,
 * pitch or frame_stride that is no multiple of 4; frame0 < 0, n_frames <= 0 or frame0 + n_frames > N; h0 or w0 not positive; reserved != 0. */
int ppms_video_colour_u8(const uint8_t* left, const uint8_t* right, int64_t frame_stride,
                         int N, int H0, int W0, int frame0, int n_frames, int x0, int y0, int h0, int w0,
                         const uint8_t* table, const ppms_egress_plane* out, void* stream);
int ppms_video_colour_u8_remap(const uint8_t* left, const uint8_t* right, int64_t frame_stride, const ppms_remap_view* lmap, const ppms_remap_view* rmap,
                               int N, int H0, int W0, int frame0, int n_frames, int x0, int y0, int h0, int w0,
                               const uint8_t* table, const ppms_egress_plane* out, void* stream);
int ppms_video_colour_yuv420(const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m,
                             int N, int H0, int W0, int frame0, int n_frames, int x0, int y0, int h0, int w0,
                             const uint8_t* table, const ppms_egress_plane* out, void* stream);
int ppms_video_colour_yuv420_remap(const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m,
                                   const ppms_remap_view* lmap, const ppms_remap_view* rmap,
                                   int N, int H0, int W0, int frame0, int n_frames, int x0, int y0, int h0, int w0,
                                   const uint8_t* table, const ppms_egress_plane* out, void* stream);
int ppms_video_colour_yuv(const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, const ppms_yuv_format* fmt,
                          int N, int H0, int W0, int frame0, int n_frames, int x0, int y0, int h0, int w0,
                          const uint8_t* table, const ppms_egress_plane* out, void* stream);
int ppms_video_colour_yuv_remap(const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, const ppms_yuv_format* fmt,
                                const ppms_remap_view* lmap, const ppms_remap_view* rmap,
                                int N, int H0, int W0, int frame0, int n_frames, int x0, int y0, int h0, int w0,
                                const uint8_t* table, const ppms_egress_plane* out, void* stream);
int ppms_video_colour_raw(const ppms_raw_view* left, const ppms_raw_view* right, const ppms_raw_format* fmt,
                          int N, int H0, int W0, int frame0, int n_frames, int x0, int y0, int h0, int w0,
                          const uint8_t* table, const ppms_egress_plane* out, void* stream);
int ppms_video_colour_raw_remap(const ppms_raw_view* left, const ppms_raw_view* right, const ppms_raw_format* fmt,
                                const ppms_remap_view* lmap, const ppms_remap_view* rmap,
                                int N, int H0, int W0, int frame0, int n_frames, int x0, int y0, int h0, int w0,
                                const uint8_t* table, const ppms_egress_plane* out, void* stream);
int ppms_video_colour_yuv_packed(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_yuv_matrix* m, const ppms_yuv_packed_format* fmt,
                                 int N, int H0, int W0, int frame0, int n_frames, int x0, int y0, int h0, int w0,
                                 const uint8_t* table, const ppms_egress_plane* out, void* stream);
int ppms_video_colour_yuv_packed_remap(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_yuv_matrix* m, const ppms_yuv_packed_format* fmt,
                                       const ppms_remap_view* lmap, const ppms_remap_view* rmap,
                                       int N, int H0, int W0, int frame0, int n_frames, int x0, int y0, int h0, int w0,
                                       const uint8_t* table, const ppms_egress_plane* out, void* stream);
int ppms_video_colour_raw_packed(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_raw_packed_format* fmt,
                                 int N, int H0, int W0, int frame0, int n_frames, int x0, int y0, int h0, int w0,
                                 const uint8_t* table, const ppms_egress_plane* out, void* stream);
int ppms_video_colour_raw_packed_remap(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_raw_packed_format* fmt,
                                       const ppms_remap_view* lmap, const ppms_remap_view* rmap,
                                       int N, int H0, int W0, int frame0, int n_frames, int x0, int y0, int h0, int w0,
                                       const uint8_t* table, const ppms_egress_plane* out, void* stream);
int ppms_video_colour_rgb_packed(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_rgb_packed_format* fmt,
                                 int N, int H0, int W0, int frame0, int n_frames, int x0, int y0, int h0, int w0,
                                 const uint8_t* table, const ppms_egress_plane* out, void* stream);
int ppms_video_colour_rgb_packed_remap(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_rgb_packed_format* fmt,
                                       const ppms_remap_view* lmap, const ppms_remap_view* rmap,
                                       int N, int H0, int W0, int frame0, int n_frames, int x0, int y0, int h0, int w0,
                                       const uint8_t* table, const ppms_egress_plane* out, void* stream);
/* nn.InstanceNorm2d(affine=False) (extractor.py:326-329, 364): per (sample, channel) mean and 1 / sqrt(biased var + eps) over the
 * HW pixels of x (channel-last fp32 [N * HW][ld], a convolution's fp32 output) -> stats[N][C][2] (pixel slices merged in fixed
 * order: deterministic; caller-owned 16-B aligned workspace of ppms_instnorm_workspace_bytes); then
 * out = relu?( (x - mean) * rstd + res? ) as split planes (res: optional residual view, e.g. relu(x + y) of extractor.py:345;
 * channels >= C of out are zeroed). */
int64_t ppms_instnorm_workspace_bytes(int N, int HW, int C);       /* per-slice partial statistics of ppms_instnorm_stats: 16 bytes per (n, slice, c) */
int ppms_instnorm_stats(const float* x, int ld, int N, int HW, int C, float eps, float* stats, void* workspace, void* stream);
int ppms_instnorm_apply(const float* x, int ld, const float* stats, ppms_sp res, int relu, ppms_sp out, int N, int HW, int C, void* stream);

/* ---------------------------------------------------------------- context encoder (cnet) pieces
 * Feature("tiny", 256) = frozen ConvNeXt-V2-tiny + FPN decoder, convnext.py:50-264.  Its Linear / conv layers
 * run on ppms_conv_gemm2 (1x1 over channel-last data; the patchify stem 4x4 s4 and the 2x2 s2 downsamplers over space-to-depth
 * copies); these are the rest:
 * ppms_dwconv: depthwise k x k conv + bias (Block.dwconv :60; k = 7), weights [C][k*k]; x split planes -> y fp32 [pixel][ldy].
 * ppms_layernorm_any: LayerNorm over the C channels of a pixel, eps given (:11-35, both data formats; 1e-6), fp32 -> split planes.
 * ppms_grn: GRN (:37-48): out = gamma * (x * Nx) + beta + x, Nx = ||x||_2 over a sample's pixels / (its mean over channels + 1e-6);
 *   x fp32 [N * HW][ld] (the GELU output), caller-owned workspace of ppms_grn_workspace_bytes; deterministic.
 * ppms_sp_upsample2: nn.Upsample(scale_factor=2) (nearest, :226-238) of a split-plane view into another (e.g. a channel range of the
 *   concatenation buffer of :259-261). */
int ppms_dwconv(ppms_sp x, float* y, int ldy, const float* w, const float* b, int k, int N, int H, int W, void* stream);
int ppms_layernorm_any(const float* x, int ld, const float* w, const float* b, float eps, ppms_sp out, int64_t pixels, int C, void* stream);
int64_t ppms_grn_workspace_bytes(int N, int HW, int C);
int ppms_grn(const float* x, int ld, const float* gamma, const float* beta, ppms_sp out, int N, int HW, int C, void* workspace, void* stream);
int ppms_sp_upsample2(ppms_sp src, ppms_sp dst, int N, int H, int W, void* stream);

/* ---------------------------------------------------------------- pick-and-play memory attention */
/* PPMStereo.compute_qk_similarity, ppmstereo.py:397-423.  q,k: fp32 [T][H*W][ld] channel-last (128 channels);
 * pooled: workspace fp32 [2][T][(H/4)*(W/4)]; sim: fp32 [T][T], sim[i][j] = cos(kbar_i, qbar_j). */
int ppms_qk_similarity(const float* q, const float* k, int ld, float* pooled, float* sim, int T, int H, int W, void* stream);
/* its two halves, for a window whose frames are sharded over GPUs: pooled descriptors of this rank's frames
 * (pooled: fp32 [2][T][(H/4)*(W/4)]), then -- after an all-gather of the descriptors -- the T x T cosine matrix */
int ppms_qk_pool(const float* q, const float* k, int ld, float* pooled, int T, int H, int W, void* stream);
int ppms_qk_cos(const float* pooled, float* sim, int T, int cells, void* stream);
/* QAM score + top-k pick + usage counter, ppmstereo.py:501-513, and the normalised play scores of :532-533.
 * conf_partial: output of ppms_unc_tail; strive: fp32 [T][T] in/out; sel: int32 [T][5] ascending frame ids;
 * shat: fp32 [T][5]; score (optional): fp32 [T][T].  1 <= T <= 64.  The pick is the min(5, T) highest scores of a row; among equal
 * scores the LOWEST frame index wins (torch's argsort leaves that order open).  Slots >= min(5, T) of sel / shat are written as 0. */
int ppms_qam_select(const float* sim, float* strive, const float* conf_partial, int nblk, int HW, int32_t* sel, float* shat,
                    float* score, int T, void* stream);
/* Q = bf16(q_i + PE_i) (ppmstereo.py:518-522); qb: bf16 [T][n][128].  ppms_attn_prep_q / ppms_attn_prep_k / ppms_pick_prep_k read q / key
 * / pe and write qb / kb 16 bytes at a time: those pointers must be 16-byte aligned (and ld % 4 == 0), T and n must be > 0; anything else
 * is refused with PPMS_EINVAL before any launch.  Each value is ONE fp32 operation (a sum; a product, then a sum: not contracted) rounded
 * to bf16. */
int ppms_attn_prep_q(const float* q, int ld, const float* pe, void* qb, int T, int n, void* stream);
/* K' = bf16(K_j * s_hat_ij + PE_j) for the picked frames (ppmstereo.py:541,547); kb: bf16 [T][ksel][n][128] */
int ppms_attn_prep_k(const float* key, int ld, const float* pe, const int32_t* sel, const float* shat, void* kb, int T, int ksel,
                     int n, void* stream);
/* ppms_qam_select + ppms_attn_prep_k as ONE launch, for a window held by one device (sel / shat / kb cover all T clips; ksel = min(5, T)):
 * the same SEL, SHAT, SCORE, counter and K', bit for bit.  The usage counter is a ping-pong pair: strive_in is read (by every workgroup),
 * strive_out -- another fp32 [T][T] table -- receives all T x T new values; the caller swaps the two after the call.  Every fp32 key is
 * read once however many clips picked its frame.  score is optional. */
int ppms_pick_prep_k(const float* sim, const float* strive_in, float* strive_out, const float* conf_partial, int nblk, int HW, int32_t* sel,
                     float* shat, float* score, const float* key, int ld, const float* pe, void* kb, int T, int n, void* stream);
enum { PPMS_ATTN_P_BF16 = 0, PPMS_ATTN_P_FP16 = 1 };   /* ppms_mem_attn: p_format */
/* flash_attn_func call of ppmstereo.py:550 for all T clips + the aggregation of :552:
 * hid = bf16(softmax(Q K'^T * scale) V); mfg = mf + beta * hid.
 * qb: bf16 [T][n][128]; kb: bf16 [T][ksel][n][128]; vt: 16-bit [T][128][n] (per-frame transposed values, picked through
 * sel; format: p_format); mf / mfg: SP views (128 channels).  out_bf16 (optional): bf16 [T][n][128] raw attention output.
 * p_format: the 16-bit format in which the unnormalised probabilities P~ = exp(S - m) enter the P~ V product on the matrix cores, and the
 * format of vt.  The reference's shim evaluates that product with fp32 P and bf16-rounded V (tools/gen_golden.py:89-95; flash-attention itself
 * rounds P~ to bf16).  PPMS_ATTN_P_BF16: P~ and vt in bf16 (8 significand bits on P~).  PPMS_ATTN_P_FP16: P~ in fp16 (11 bits), vt = the fp16
 * image of the bf16-rounded values (ppms_epilogue.vt_f16 = 1): V is still "cast to bf16" as ppmstereo.py:550 does, Q K'^T is computed on
 * bf16 operands either way, the MFMA count is the same -- an eighth of the P~ rounding error (what keeps the iters = 20 cascade inside 1e-3 px).
 * mf.hi == NULL: no aggregation -- the `mfg` view receives hid itself (hi plane = hid, lo plane = 0: bf16-exact channels, see
 * ppms_conv.lo_zero_from; the caller then feeds the convolutions [mf | hid] with weights (W_mf + W_mfg | beta W_mfg), the same sum).
 * Alignment: qb, kb, out_bf16, split_ws and the four planes of mf / mfg are accessed 16 bytes at a time and must be 16-byte aligned (views: a
 * multiple of 8 channels, ld % 8 == 0); so must vt where n % 8 == 0 (other n read it element by element).  A call that is not is refused with
 * PPMS_EINVAL before any launch.  sel rows hold frame indices into vt, which may hold more frames than the T clips of the call (a sharded
 * window: T clips of this rank, all frames of the window). */
int ppms_mem_attn(const void* qb, const void* kb, const void* vt, const int32_t* sel, int ksel, float scale, const float* beta,
                  ppms_sp mf, ppms_sp mfg, void* out_bf16, int T, int n, void* split_ws, int frames_per_workgroup, int p_format, void* stream);
/* split_ws (optional, caller-owned, ppms_mem_attn_workspace_bytes(T, ksel, n) bytes, contents need not be
 * initialised): when given, every picked frame (or pair of picked frames) is processed by its own workgroups, which leave fp32 partials
 * (O, m, l) in the workspace, and a combine kernel merges them; with n % 64 == 0 this is the 64-queries-per-wave
 * LDS-DMA kernel (rescale-free accumulation + a fix-up pass for tiles it flags -- scores more than 2^60 (bf16 P~) / 2^16 (fp16 P~) above
 * the softmax reference of their query, see mem_attn.hip).  NULL = one fused
 * launch of the 32-query online-softmax kernel.
 * frames_per_workgroup: the 64-query kernel gives a workgroup ONE picked frame, or TWO consecutive ones where the one-frame grid would
 * run at least two rounds on the chip (fewer partials to write and combine).  0 = the library's choice (1 or 2), 1 .. 5 = this call uses that
 * many (5 = all picked frames in one workgroup: one partial set per clip; a per-call argument: the library keeps no mutable state).  The
 * same softmax either way (different summation order). */
int64_t ppms_mem_attn_workspace_bytes(int T, int ksel, int n);
/* The number of frame splits (partial sets per clip) ppms_mem_attn uses for these arguments when it is given a workspace: the launch's own
 * planner, evaluated without launching.  frames_per_workgroup 1 .. 5: ceil(ksel / frames_per_workgroup); 0: the library's choice on the
 * current device.  0 when the 64-query kernel does not serve the geometry (n % 64 != 0: no redo flags are written); PPMS_EINVAL on
 * arguments ppms_mem_attn refuses. */
int ppms_mem_attn_splits(int T, int ksel, int n, int frames_per_workgroup);
/* Fix-up accounting of the 64-query kernel, counted on the device: enqueued on `stream` behind a ppms_mem_attn call that used the same
 * split_ws, T, ksel, n and frames_per_workgroup, it reads the T * nsp * ceil(n / 256) redo flag pairs that call wrote (nsp =
 * ppms_mem_attn_splits; one pair per (clip, split, 256-query block) tile) -- no other byte of the workspace, and it writes none -- and adds
 * to counters (caller-owned device memory, int64 [3], zeroed by the caller): {calls += 1, tiles += T * nsp * ceil(n / 256), flagged +=
 * tiles the fix-up pass recomputed}.  One small launch; no allocation, no host synchronisation: the caller reads the counters when it
 * synchronises anyway.  Returns 0 without launching when ppms_mem_attn_splits is 0. */
int ppms_attn_redo_accumulate(const void* split_ws, int T, int ksel, int n, int frames_per_workgroup, int64_t* counters, void* stream);

/* Fused chain of up to three per-pixel (1x1, <= 64 input channels) layers with GELU, optional residual from the chain
 * input and optional depthwise-1x1 post step: the ffn1 / pw / ffn2 parts of PCBlock4_Deep_nopool_res
 * (ppmtereo_update.py:1024-1030).  dev_params: device copy of the parameter block built by the host
 * (ppmstereo_amd/engine.py: PwChain; layout checked with ppms_pwchain_param_bytes).  The input view is read 64 channels wide (channels
 * beyond a layer's real inputs meet zero weights: they must hold finite values).  Of the last layer only channels [0, n_valid) of the
 * `pixels` rows are stored: channels >= n_valid of the output view (its padding up to M) and rows >= pixels are NOT written -- they keep
 * what the buffer held (a caller that feeds them to a convolution zeroes the buffer once).  Maps of <= 16 384 pixels run a 32-pixel-tile
 * kernel, larger ones a 128-pixel-tile kernel: the same bits per pixel either way. */
int ppms_pwchain(const void* dev_params, int64_t pixels, void* stream);
int ppms_pwchain_param_bytes(void);

/* ---------------------------------------------------------------- update_block16 time / space attention pieces */
/* TimeAttnBlock core (ppmtereo_update.py:603-606 with Attention.forward :409-417): per pixel, tokens = its T frames;
 * y = LayerNorm(x); out_t = sum_t2 softmax(y_t . y_t2 / sqrt(C / 8)) y_t2 per head (q = k = v = y; 8 heads).  x, out: SP, 384 channels
 * (update_block16) or 256 (the SST block's TimeAttnBlock, ppmstereo.py:392-393).  A pixel's T normalised frames are held in T * C * 4 bytes of
 * LDS, at most 64 KiB: T <= 42 at C = 384, T <= 64 at C = 256; a larger T is refused with PPMS_EINVAL before any launch. */
int ppms_time_attn(ppms_sp x, const float* ln_w, const float* ln_b, ppms_sp out, int T, int n, int heads, void* stream);
/* out = resid + LayerNorm(x) (resid.hi == NULL: no residual); x fp32 [pixel][ld]; C = 384 or 256 (attention.py:186-190) */
int ppms_layernorm(const float* x, int ld, const float* w, const float* b, ppms_sp resid, ppms_sp out, int64_t pixels, int C, void* stream);
/* LinearAttention.forward (attention.py:73-100) per frame and head: Q, K already elu()+1, V already / n;
 * kv_ws: fp32 workspace of ppms_linear_attention_workspace_floats(T, n, heads, dh) floats (the per-pixel-split partial sums);
 * out (SP) = (Q KV) / (Q . sum K + 1e-6) * n */
int64_t ppms_linear_attention_workspace_floats(int T, int n, int heads, int dh);
int ppms_linear_attention(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* kv_ws, ppms_sp out, int T, int n,
                          int heads, int dh, void* stream);

#ifdef __cplusplus
}
#endif
#endif
