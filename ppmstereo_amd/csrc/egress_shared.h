// What the egress sources (egress.hip: the planes and the organised points; cloud_egress.hip: the compacted cloud; normals_egress.hip: the
// normals plane and the oriented cloud, which is built from the compacted cloud's pieces at the end of this file) share: the thread mapping,
// the loads of the engine's state, and the host checks of the geometry and the frame range, of the reprojection's arguments and of a strided
// destination.  Device pieces are restated nowhere else: a pixel's d and u are the same bits whichever launch reads them.  The check of a
// colour plane (4-byte pixels) is here too: video_ingest.hip's colour kernel writes such a plane, cloud_egress.hip's coloured cloud reads it.
#pragma once
#include "common.h"

// one thread = a run of EG_RUN consecutive x of one output row
constexpr int EG_RUN = 8;
// bilinear_kernel's expression for output pixel (oy, ox) of one H x W source plane `s`, align_corners = 0, restated (every operation is one
// fp32 operation in the same order, and the build contracts nothing: the same bits as ppms_bilinear with mul = 1).  bilinear_kernel does not
// call it: routed through this function its instructions come out in another order, and its generated code is kept as it is.
__device__ __forceinline__ float bilinear_tap(const float* __restrict__ s, int H, int W, float sh, float sw, int oy, int ox) {
    const float fy = fmaxf(sh * (oy + 0.5f) - 0.5f, 0.0f);
    const float fx = fmaxf(sw * (ox + 0.5f) - 0.5f, 0.0f);
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + ((y0 < H - 1) ? 1 : 0), x1 = x0 + ((x0 < W - 1) ? 1 : 0);
    const float ly = fy - y0, lx = fx - x0;
    const float hy = 1.0f - ly, hx = 1.0f - lx;
    return hy * (hx * s[y0 * W + x0] + lx * s[y0 * W + x1]) + ly * (hx * s[y1 * W + x0] + lx * s[y1 * W + x1]);
}
// ---- the pieces every egress kernel is built from
// thread idx -> its run: n elements from column x0 of row y of output frame `frame`; (sy, sx) = the run's first pixel in the padded H x W frame
struct egress_run { int x0, y, n, sy, sx; int64_t frame; };
__device__ __forceinline__ egress_run egress_map(int64_t idx, int rpr, int H0, int W0, int pad_left, int pad_top) {
    egress_run r;
    r.x0 = (int)(idx % rpr) * EG_RUN;
    const int64_t row = idx / rpr;                                       // frame * H0 + y of the output
    r.y = (int)(row % H0);
    r.frame = row / H0;
    r.n = W0 - r.x0 < EG_RUN ? W0 - r.x0 : EG_RUN;                       // elements of this run inside the row
    r.sy = r.y + pad_top, r.sx = r.x0 + pad_left;
    return r;
}
// d = |flow_up[frame0 + frame, 0]| over the run (past the row's end the last element again)
__device__ __forceinline__ void egress_load_disparity(const float* __restrict__ flow_up, int H, int W, int frame0, const egress_run& r,
                                                      float (&d)[EG_RUN]) {
    const float* s = flow_up + ((frame0 + r.frame) * 2 * H + r.sy) * W + r.sx;      // channel 0 of (T, 2, H, W)
    if (r.n == EG_RUN && ((uintptr_t)s & 15) == 0) {
        const f32x4 a = gld<f32x4>(s), b = gld<f32x4>(s + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            d[j] = a[j];
            d[4 + j] = b[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < EG_RUN; ++j) d[j] = s[j < r.n ? j : r.n - 1];
    }
#pragma unroll
    for (int j = 0; j < EG_RUN; ++j) d[j] = fabsf(d[j]);
}
// u = |the 4x bilinear upsampling of unc[frame0 + frame]| over the run
__device__ __forceinline__ void egress_load_uncertainty(const float* __restrict__ unc, int H, int W, int frame0, float sh, float sw,
                                                        const egress_run& r, float (&u)[EG_RUN]) {
    const int h = H / 4, w = W / 4;
    const float* s = unc + (frame0 + r.frame) * h * w;
#pragma unroll
    for (int j = 0; j < EG_RUN; ++j) u[j] = fabsf(bilinear_tap(s, h, w, sh, sw, r.sy, r.sx + (j < r.n ? j : r.n - 1)));
}
// ---- host: the geometry and the frame range every egress entry point refuses alike, under the name `who` of the one called.  On success
// the launch geometry: runs per output row, runs in all (one thread each), ppms_bilinear's scales for (H/4, W/4) -> (H, W).
struct egress_launch { int rpr; int64_t total; float sh, sw; };
static inline int egress_check_geometry(const char* who, int T, int H, int W, int frame0, int n_frames, int pad_left, int pad_top, int H0, int W0,
                                        egress_launch* g) {
    PPMS_REQUIRE(T > 0 && H > 0 && W > 0 && H0 > 0 && W0 > 0, "%s: T = %d, H = %d, W = %d, H0 = %d, W0 = %d must be positive", who, T, H, W, H0, W0);
    PPMS_REQUIRE(H % 4 == 0 && W % 4 == 0, "%s: H = %d, W = %d must be multiples of 4", who, H, W);
    PPMS_REQUIRE(pad_left >= 0 && pad_top >= 0 && (int64_t)pad_top + H0 <= H && (int64_t)pad_left + W0 <= W,
                 "%s: the crop pad_left = %d, pad_top = %d, H0 = %d, W0 = %d lies outside the %d x %d frame", who, pad_left, pad_top, H0, W0, H, W);
    PPMS_REQUIRE(n_frames > 0, "%s: n_frames = %d must be positive", who, n_frames);
    PPMS_REQUIRE(frame0 >= 0 && (int64_t)frame0 + n_frames <= T, "%s: frame0 = %d, n_frames = %d leave the T = %d frames", who, frame0, n_frames, T);
    g->rpr = (W0 + EG_RUN - 1) / EG_RUN;                                 // runs per output row
    g->total = (int64_t)n_frames * H0 * g->rpr;
    PPMS_REQUIRE((g->total + 255) / 256 <= 0x7fffffff, "%s: %lld threads exceed one grid", who, (long long)g->total);
    g->sh = (float)(H / 4) / (float)H, g->sw = (float)(W / 4) / (float)W;            // ppms_bilinear's scales for (H/4, W/4) -> (H, W): 0.25
    return PPMS_OK;
}
// ---- host: the reprojection's arguments, as ppms_scene_egress and ppms_cloud_egress refuse them.  The gates' values always; q and min_disp
// where records are made (`records`: points or a cloud, of `components` each); unc where a gate that something obeys (`gated`: a depth plane or
// records) or a fourth component reads it.
static inline int egress_check_reprojection(const char* who, const float* unc, const float (&q)[16], float min_disp, float max_uncertainty,
                                            float max_depth, bool records, bool gated, int components) {
    PPMS_REQUIRE(max_uncertainty == max_uncertainty, "%s: max_uncertainty is NaN (+inf switches the gate off)", who);
    PPMS_REQUIRE(max_depth > 0.0f, "%s: max_depth = %g must be positive (+inf switches the gate off)", who, (double)max_depth);
    if (records) {
        for (int i = 0; i < 16; ++i) PPMS_REQUIRE(q[i] > -INFINITY && q[i] < INFINITY, "%s: q[%d] = %g is not finite", who, i, (double)q[i]);
        PPMS_REQUIRE(min_disp > -INFINITY && min_disp < INFINITY, "%s: the reprojection needs a finite min_disp, got %g", who, (double)min_disp);
    }
    const bool reads_u = (gated && max_uncertainty < INFINITY) || (records && components == 4);
    PPMS_REQUIRE(!reads_u || unc != nullptr, "%s: null unc: the max_uncertainty gate and a fourth component read it", who);
    return PPMS_OK;
}
// ---- host: a strided destination `name`: n_frames frames frame_stride bytes apart, each `rows` rows *pitch bytes apart of row_elems elements
// of `format` (PPMS_FMT_F32: 4 bytes, PPMS_FMT_U8: 1, otherwise 2).  pitch == nullptr: a frame is one dense row (the cloud's records and
// indices).  stride_name: what the caller's struct calls frame_stride.
static inline int egress_check_strided(const char* who, const char* name, const char* stride_name, const void* ptr, int64_t frame_stride,
                                       const int64_t* pitch, int format, int n_frames, int64_t rows, int64_t row_elems) {
    const int64_t esz = format == PPMS_FMT_F32 ? 4 : (format == PPMS_FMT_U8 ? 1 : 2), rowb = esz * row_elems, step = pitch ? *pitch : rowb;
    PPMS_REQUIRE(step >= rowb, "%s: %s.pitch = %lld is less than a row's %lld bytes", who, name, (long long)step, (long long)rowb);
    PPMS_REQUIRE(n_frames == 1 || frame_stride >= (rows - 1) * step + rowb, "%s: %s = %lld is less than a frame's %lld bytes", who, stride_name,
                 (long long)frame_stride, (long long)((rows - 1) * step + rowb));
    PPMS_REQUIRE(((uintptr_t)ptr | (uintptr_t)step | (uintptr_t)frame_stride) % esz == 0,
                 "%s: %s: pointer, pitch and %s must be multiples of the %lld-byte element", who, name, stride_name, (long long)esz);
    return PPMS_OK;
}
// ---- host: a colour plane (PPMS_FMT_RGBA8 / PPMS_FMT_BGRA8: 4-byte pixels) of n_frames x rows x cols pixels, as ppms_video_colour_* (the plane it
// writes) and ppms_cloud_egress_colour (the plane it reads) refuse it; `name`: what the message calls the plane
static inline int egress_check_colour_plane(const char* who, const char* name, const ppms_egress_plane* p, int n_frames, int64_t rows, int64_t cols) {
    PPMS_REQUIRE(p && p->ptr, "%s: null %s plane", who, name);
    PPMS_REQUIRE(p->format == PPMS_FMT_RGBA8 || p->format == PPMS_FMT_BGRA8, "%s: %s.format = %d is neither PPMS_FMT_RGBA8 nor PPMS_FMT_BGRA8", who, name,
                 p->format);
    PPMS_REQUIRE(p->reserved == 0, "%s: %s.reserved = %d must be 0", who, name, p->reserved);
    char stride[64];
    snprintf(stride, sizeof(stride), "%s.frame_stride", name);
    return egress_check_strided(who, name, stride, p->ptr, p->frame_stride, &p->pitch, PPMS_FMT_F32, n_frames, rows, cols);      // (4-byte elements)
}
// ---- the compact clouds' pieces (cloud_egress.hip: ppms_cloud_egress and its coloured twin; normals_egress.hip: the oriented cloud).  A workgroup
// of WG threads takes WG consecutive runs of ONE frame with egress_map's mapping, so thread order is row-major pixel order.
constexpr int CLOUD_WG = 256;
constexpr int CLOUD_PIXELS = CLOUD_WG * EG_RUN;                          // pixels of a workgroup: the most records it places (2048)

// d, u (where a gate or w reads it), X, Y, Z of the run's pixels; returns the validity mask, bit j = pixel j of the run (0 past the row's end).
// scene_egress_kernel's arithmetic, restated: that kernel does not call this function, its generated code stays as it is.
__device__ __forceinline__ unsigned cloud_points(const float* __restrict__ flow_up, const float* __restrict__ unc, const ppms_cloud& c, bool want_w,
                                                 int H, int W, int frame0, float sh, float sw, const egress_run& r, float (&X)[EG_RUN],
                                                 float (&Y)[EG_RUN], float (&Z)[EG_RUN], float (&u)[EG_RUN]) {
    const bool gate_u = c.max_uncertainty < INFINITY, gate_z = c.max_depth < INFINITY;
    if (gate_u || want_w) {
        egress_load_uncertainty(unc, H, W, frame0, sh, sw, r, u);
    } else {
#pragma unroll
        for (int j = 0; j < EG_RUN; ++j) u[j] = 0.0f;
    }
    float d[EG_RUN];
    egress_load_disparity(flow_up, H, W, frame0, r, d);
    const float yf = (float)r.y;                                          // the pixel's row and column in the cropped plane
    float qy[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qy[i] = c.q[4 * i + 1] * yf;
    unsigned mask = 0;
#pragma unroll
    for (int j = 0; j < EG_RUN; ++j) {
        const bool ok = d[j] >= c.min_disp && (!gate_u || u[j] <= c.max_uncertainty);     // valid_d and valid_u (both false for NaN)
        const float xf = (float)(r.x0 + j);
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = ((c.q[4 * i] * xf + qy[i]) + c.q[4 * i + 2] * d[j]) + c.q[4 * i + 3];
        const float pz = __fdiv_rn(v[2], v[3]);
        const bool okp = ok && (!gate_z || (pz > 0.0f && pz <= c.max_depth));
        X[j] = __fdiv_rn(v[0], v[3]);
        Y[j] = __fdiv_rn(v[1], v[3]);
        Z[j] = pz;
        mask |= (okp && j < r.n) ? 1u << j : 0u;
    }
    return mask;
}
// the thread's run of frame blockIdx.y (ridx: its number inside the frame) and its points; an idle thread past the frame's last run has no pixel
template <int WG = CLOUD_WG>
__device__ __forceinline__ unsigned cloud_thread(const float* __restrict__ flow_up, const float* __restrict__ unc, const ppms_cloud& c, bool want_w,
                                                 int H, int W, int frame0, int pad_left, int pad_top, int H0, int W0, float sh, float sw, int rpr,
                                                 int64_t runs, egress_run& r, float (&X)[EG_RUN], float (&Y)[EG_RUN], float (&Z)[EG_RUN],
                                                 float (&u)[EG_RUN]) {
    const int64_t ridx = (int64_t)blockIdx.x * WG + threadIdx.x;
    if (ridx >= runs) return 0u;
    r = egress_map((int64_t)blockIdx.y * runs + ridx, rpr, H0, W0, pad_left, pad_top);
    return cloud_points(flow_up, unc, c, want_w, H, W, frame0, sh, sw, r, X, Y, Z, u);
}
// exclusive prefix sum of v over the workgroup's WG threads in thread order, and the workgroup's total: a wave64 scan, then the waves'
// totals through LDS (ws: WG / 64 ints).  Integer sums in a fixed order; ws may be used again after the call.
struct cloud_scan { int before, total; };
template <int WG = CLOUD_WG>
__device__ __forceinline__ cloud_scan cloud_block_scan(int v, int* ws) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int s = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(s, off);
        if (lane >= off) s += t;
    }
    if (lane == 63) ws[wave] = s;
    __syncthreads();
    cloud_scan out;
    out.before = s - v;
    out.total = 0;
#pragma unroll
    for (int i = 0; i < WG / 64; ++i) {
        if (i < wave) out.before += ws[i];
        out.total += ws[i];
    }
    __syncthreads();
    return out;
}
// The workgroup's staged bytes [lo, hi) of `smem` -> global `gbase + the same offset`.  smem and gbase are congruent mod 16 (the staging is
// shifted by the destination's misalignment), so the whole 16-byte slots inside the range go out as 16-byte stores; the head in front of the
// first whole slot and the tail behind the last one element by element (E: the element, which lo and hi are multiples of).
template <class E, int WG = CLOUD_WG>
__device__ __forceinline__ void cloud_flush(const char* smem, char* gbase, int lo, int hi) {
    int first = (lo + 15) & ~15, last = hi & ~15;
    if (last < first) first = last = hi;                                 // no whole slot: all of it element by element
    for (int off = first + (int)threadIdx.x * 16; off < last; off += WG * 16) gstore16(gbase + off, *(const u32x4*)(smem + off));
    const int head = (first - lo) / (int)sizeof(E), tail = (hi - last) / (int)sizeof(E);         // fewer than 16 / sizeof(E) elements each
    if ((int)threadIdx.x < head) *(E*)(gbase + lo + threadIdx.x * sizeof(E)) = *(const E*)(smem + lo + threadIdx.x * sizeof(E));
    if ((int)threadIdx.x < tail) *(E*)(gbase + last + threadIdx.x * sizeof(E)) = *(const E*)(smem + last + threadIdx.x * sizeof(E));
}
// workgroups of `wg` threads per frame; 0 for a geometry the entry points refuse
static inline int64_t cloud_blocks_per_frame(int H0, int W0, int wg = CLOUD_WG) {
    if (H0 <= 0 || W0 <= 0 || (int64_t)H0 * W0 > 0x7fffffff) return 0;
    return ((int64_t)H0 * ((W0 + EG_RUN - 1) / EG_RUN) + wg - 1) / wg;
}
// ---- host: what the compact clouds' entry points check, under the name `who` of the one called; on success the launch geometry and the workgroups
// per frame.  layout: what a record holds beside X, Y, Z -- CLOUD_PLAIN (ppms_cloud_egress: 3 or 4 components, the fourth u), CLOUD_COLOUR
// (ppms_cloud_egress_colour: the fourth component is the colour word, so nothing but the max_uncertainty gate reads unc), CLOUD_NORMALS
// (ppms_cloud_egress_normals: 6 or 7 components, workgroups of `wg` threads; unc as for CLOUD_COLOUR)
enum { CLOUD_PLAIN = 0, CLOUD_COLOUR = 1, CLOUD_NORMALS = 2 };
static inline int cloud_check(const char* who, const float* flow_up, const float* unc, int T, int H, int W, int frame0, int n_frames, int pad_left,
                              int pad_top, int H0, int W0, const ppms_cloud* out, int layout, egress_launch& g, int64_t* blocks_out, int wg = CLOUD_WG) {
    PPMS_REQUIRE(out, "%s: null out struct", who);
    const ppms_cloud& c = *out;
    if (const int rc = egress_check_geometry(who, T, H, W, frame0, n_frames, pad_left, pad_top, H0, W0, &g)) return rc;
    PPMS_REQUIRE((int64_t)H0 * W0 <= 0x7fffffff, "%s: H0 * W0 = %lld pixel indices exceed int32", who, (long long)H0 * W0);
    PPMS_REQUIRE(n_frames <= 65535, "%s: n_frames = %d exceeds one grid", who, n_frames);
    PPMS_REQUIRE(flow_up != nullptr, "%s: null flow_up", who);
    PPMS_REQUIRE(c.records != nullptr, "%s: null records", who);
    PPMS_REQUIRE(c.counts != nullptr, "%s: null counts", who);
    PPMS_REQUIRE(c.format == PPMS_FMT_F32 || c.format == PPMS_FMT_F16, "%s: format = %d is neither PPMS_FMT_F32 nor PPMS_FMT_F16", who, c.format);
    if (layout == CLOUD_NORMALS)
        PPMS_REQUIRE(c.components == 6 || c.components == 7, "%s: components = %d must be 6 or 7", who, c.components);
    else
        PPMS_REQUIRE(c.components == 3 || c.components == 4, "%s: components = %d must be 3 or 4", who, c.components);
    PPMS_REQUIRE(c.reserved == 0, "%s: reserved = %d must be 0", who, c.reserved);
    PPMS_REQUIRE(c.capacity > 0 && c.capacity <= 0x7fffffff, "%s: capacity = %lld must be in 1 .. 2^31 - 1", who, (long long)c.capacity);
    // a frame of records, and of indices (int32: 4-byte elements, as PPMS_FMT_F32 has), is one dense row of `capacity` of them
    if (const int rc = egress_check_strided(who, "records", "frame_stride", c.records, c.frame_stride, nullptr, c.format, n_frames, 1, c.capacity * c.components))
        return rc;
    if (c.index)
        if (const int rc = egress_check_strided(who, "index", "index_frame_stride", c.index, c.index_frame_stride, nullptr, PPMS_FMT_F32, n_frames, 1, c.capacity))
            return rc;
    PPMS_REQUIRE((uintptr_t)c.counts % 4 == 0 && (uintptr_t)c.block_counts % 4 == 0, "%s: counts and block_counts must be multiples of the 4-byte element", who);
    const int64_t blocks = cloud_blocks_per_frame(H0, W0, wg);
    PPMS_REQUIRE(c.block_counts != nullptr && c.block_counts_len >= n_frames * blocks,
                 "%s: block_counts is null or block_counts_len = %lld is less than the %lld entries of %s", who,
                 (long long)c.block_counts_len, (long long)(n_frames * blocks),
                 layout == CLOUD_NORMALS ? "ppms_cloud_egress_normals_workspace" : "ppms_cloud_egress_workspace");
    *blocks_out = blocks;
    return egress_check_reprojection(who, unc, c.q, c.min_disp, c.max_uncertainty, c.max_depth, true, true, layout == CLOUD_PLAIN ? c.components : 3);
}
