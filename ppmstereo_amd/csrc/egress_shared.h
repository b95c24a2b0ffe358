// What the egress sources share (egress.hip: the planes and the organised points; cloud_egress.hip: the compact clouds, plain, coloured and
// oriented; normals_egress.hip: the normals plane): the thread mapping, the loads of the engine's state, the one point (egress_points: the
// reprojection of a pixel and its validity), the one store of a run of records to a plane, and the host checks of the geometry and the frame
// range, of the reprojection's arguments, of a strided destination and of the two planes a cloud reads.  Device pieces are restated nowhere
// else: a pixel's d, u and point are the same bits whichever launch forms them.  (video_ingest.hip's colour kernel writes the colour plane
// that is checked here.)
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
// valid_d and valid_u of a pixel (both false for NaN); u is read only with the gate on.  scene_egress_kernel's depth plane asks it.
// egress_points holds the same line inside its loop and does not call this: with the call there, the code of every kernel that inlines the
// loop comes out differently, and the loop keeps the form it was timed in (docs/LOG_r25.md, section 6).
__device__ __forceinline__ bool egress_valid(float d, float u, float min_disp, float max_uncertainty) {
    return d >= min_disp && (!(max_uncertainty < INFINITY) || u <= max_uncertainty);
}
// The one point (include/ppms.h: the formulas): pixels (x0 + j, y), j < N, of the cropped plane with disparities d -> X, Y, Z, computed whatever
// the validity.  Returns the validity mask: bit j = valid_d, valid_u and the depth gate on Z of pixel j, and 0 for j >= n (the pixels of a run
// inside its row).  N = EG_RUN: a thread's run; N = 1: one pixel.  Every operation is one fp32 operation in the documented order and the build
// contracts nothing, so scene_egress_kernel's points plane, the clouds' records and the normals' stencil see the same bits.  The gates are
// fields of the launch's struct: every branch on them is wave-uniform.  (A run at a time, with the row's products in front of the loop: formed
// pixel by pixel the clouds' launches took 3 % longer.)
template <int N>
__device__ __forceinline__ unsigned egress_points(const float (&q)[16], float min_disp, float max_uncertainty, float max_depth, int x0, int y, int n,
                                                  const float (&d)[N], const float (&u)[N], float (&X)[N], float (&Y)[N], float (&Z)[N]) {
    const bool gate_u = max_uncertainty < INFINITY, gate_z = max_depth < INFINITY;
    const float yf = (float)y;                                           // the pixel's row and column in the cropped plane
    float qy[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qy[i] = q[4 * i + 1] * yf;
    unsigned mask = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const bool ok = d[j] >= min_disp && (!gate_u || u[j] <= max_uncertainty);     // valid_d and valid_u (both false for NaN)
        const float xf = (float)(x0 + j);
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = ((q[4 * i] * xf + qy[i]) + q[4 * i + 2] * d[j]) + q[4 * i + 3];
        const float pz = __fdiv_rn(v[2], v[3]);
        const bool okp = ok && (!gate_z || (pz > 0.0f && pz <= max_depth));
        X[j] = __fdiv_rn(v[0], v[3]);
        Y[j] = __fdiv_rn(v[1], v[3]);
        Z[j] = pz;
        mask |= (okp && j < n) ? 1u << j : 0u;
    }
    return mask;
}
// one pixel through the same body
__device__ __forceinline__ bool egress_point(const float (&q)[16], float min_disp, float max_uncertainty, float max_depth, int x, int y, float d, float u,
                                             float& X, float& Y, float& Z) {
    const float d1[1] = {d}, u1[1] = {u};
    float X1[1], Y1[1], Z1[1];
    const unsigned ok = egress_points<1>(q, min_disp, max_uncertainty, max_depth, x, y, 1, d1, u1, X1, Y1, Z1);
    X = X1[0], Y = Y1[0], Z = Z1[0];
    return ok != 0;
}
// The one store: a run of EG_RUN records of C elements each -> plane `p` at (frame, y, x0), n of them inside the row.  16 bytes at a time (8
// for a run of bytes) where the run is whole and its address allows it, element by element otherwise.
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
template <class T, int C = 1>
__device__ __forceinline__ void egress_store_run(const ppms_egress_plane& p, int64_t frame, int y, int x0, int n, const T (&v)[EG_RUN * C]) {
    T* dst = (T*)((char*)p.ptr + frame * p.frame_stride + (int64_t)y * p.pitch) + (int64_t)x0 * C;
    constexpr int BYTES = (int)sizeof(T) * EG_RUN * C;                   // 8 (a u8 plane) to 128 (f32 points with w)
    constexpr int CHUNK = BYTES < 16 ? BYTES : 16;
    if (n == EG_RUN && ((uintptr_t)dst & (CHUNK - 1)) == 0) {
        if constexpr (BYTES < 16) {
            gst<u32x2>(dst, __builtin_bit_cast(u32x2, v));
        } else {
            struct chunks { u32x4 q[BYTES / 16]; };
            const chunks c = __builtin_bit_cast(chunks, v);
#pragma unroll
            for (int i = 0; i < BYTES / 16; ++i) gstore16((char*)dst + 16 * i, c.q[i]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < EG_RUN * C; ++j)
            if (j < n * C) dst[j] = v[j];
    }
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
// ---- host: a normals plane of n_frames x H0 rows of W0 * 3 elements, as ppms_normals_egress (the plane it writes) and ppms_cloud_egress_normals
// (the plane it reads) refuse it
static inline int egress_check_normals_plane(const char* who, const ppms_egress_plane* p, int n_frames, int H0, int W0) {
    PPMS_REQUIRE(p && p->ptr, "%s: null normals plane", who);
    PPMS_REQUIRE(p->format == PPMS_FMT_F32 || p->format == PPMS_FMT_F16, "%s: normals.format = %d is neither PPMS_FMT_F32 nor PPMS_FMT_F16", who, p->format);
    PPMS_REQUIRE(p->reserved == 0, "%s: normals.reserved = %d must be 0", who, p->reserved);
    return egress_check_strided(who, "normals", "normals.frame_stride", p->ptr, p->frame_stride, &p->pitch, p->format, n_frames, H0, (int64_t)W0 * 3);
}
