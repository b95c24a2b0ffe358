// Output egress (ppmstereo_amd/engine.py: disparity_egress, driven by output.py's OutputSpec): the two one-launch-per-window kernels that
// write the caller's disparity / depth / uncertainty planes and the point cloud, their conversions, checks and entry points.  The thread mapping,
// the loads, the point, the store of a run and the geometry check are egress_shared.h's: cloud_egress.hip and normals_egress.hip are built from
// the same ones.
#include "egress_shared.h"

// ------------------------------------------------------------------------------------------------ disparity egress
// The 1/4-scale engine's state after its last iteration -> the caller's output planes, one launch (include/ppms.h: the formulas):
// crop (InputPadder.unpad), frame range, |flow_up[:, 0]|, the 4x bilinear upsampling of the uncertainty, depth = fb / d and the
// conversions to the planes' formats.  HBM bound: one thread = a run of EG_RUN consecutive x of one output row; the run is loaded
// and stored 16 bytes at a time (8 for a run of bytes) where its address allows it, element by element at row ends and on
// rows that start unaligned.  Every offset is 64-bit.  (EG_RUN, bilinear_tap, egress_map, the two loads and egress_store_run: egress_shared.h.)
// min(top, rint(v)) for v >= 0 (a magnitude times a positive scale); NaN -> 0
__device__ __forceinline__ unsigned egress_quant(float v, float top) {
    const float r = rintf(v);
    return r != r ? 0u : (unsigned)fminf(r, top);
}
__device__ __forceinline__ void egress_store_disparity(const ppms_egress& o, const egress_run& r, const float (&d)[EG_RUN]) {
    if (o.disparity.format == PPMS_FMT_F32) {
        egress_store_run(o.disparity, r.frame, r.y, r.x0, r.n, d);
    } else if (o.disparity.format == PPMS_FMT_F16) {
        _Float16 v[EG_RUN];
#pragma unroll
        for (int j = 0; j < EG_RUN; ++j) v[j] = (_Float16)d[j];
        egress_store_run(o.disparity, r.frame, r.y, r.x0, r.n, v);
    } else {
        uint16_t v[EG_RUN];
#pragma unroll
        for (int j = 0; j < EG_RUN; ++j) v[j] = (uint16_t)egress_quant(d[j] * o.disp_scale, 65535.0f);
        egress_store_run(o.disparity, r.frame, r.y, r.x0, r.n, v);
    }
}
// z and its validity come from the caller (the gates differ between the kernels): z = +inf where !ok
__device__ __forceinline__ void egress_store_depth(const ppms_egress& o, const egress_run& r, const float (&z)[EG_RUN], const bool (&ok)[EG_RUN]) {
    if (o.depth.format == PPMS_FMT_F32) {
        egress_store_run(o.depth, r.frame, r.y, r.x0, r.n, z);
    } else if (o.depth.format == PPMS_FMT_F16) {
        _Float16 v[EG_RUN];
#pragma unroll
        for (int j = 0; j < EG_RUN; ++j) v[j] = (_Float16)z[j];
        egress_store_run(o.depth, r.frame, r.y, r.x0, r.n, v);
    } else {
        uint16_t v[EG_RUN];
#pragma unroll
        for (int j = 0; j < EG_RUN; ++j) v[j] = ok[j] ? (uint16_t)egress_quant(z[j] * o.depth_scale, 65535.0f) : (uint16_t)0;
        egress_store_run(o.depth, r.frame, r.y, r.x0, r.n, v);
    }
}
__device__ __forceinline__ void egress_store_uncertainty(const ppms_egress& o, const egress_run& r, const float (&u)[EG_RUN]) {
    if (o.uncertainty.format == PPMS_FMT_F32) {
        egress_store_run(o.uncertainty, r.frame, r.y, r.x0, r.n, u);
    } else {
        uint8_t v[EG_RUN];
#pragma unroll
        for (int j = 0; j < EG_RUN; ++j) v[j] = (uint8_t)egress_quant(u[j] * 255.0f, 255.0f);
        egress_store_run(o.uncertainty, r.frame, r.y, r.x0, r.n, v);
    }
}
__global__ __launch_bounds__(256) void disparity_egress_kernel(const float* __restrict__ flow_up, const float* __restrict__ unc, ppms_egress o,
                                                                int H, int W, int frame0, int pad_left, int pad_top, int H0, int W0, float sh,
                                                                float sw, int rpr, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const egress_run r = egress_map(idx, rpr, H0, W0, pad_left, pad_top);
    if (o.disparity.ptr || o.depth.ptr) {
        float d[EG_RUN];
        egress_load_disparity(flow_up, H, W, frame0, r, d);
        if (o.disparity.ptr) egress_store_disparity(o, r, d);
        if (o.depth.ptr) {
            float z[EG_RUN];
            bool ok[EG_RUN];
#pragma unroll
            for (int j = 0; j < EG_RUN; ++j) {
                ok[j] = d[j] >= o.min_disp;                              // false for NaN
                z[j] = ok[j] ? __fdiv_rn(o.fb, d[j]) : INFINITY;
            }
            egress_store_depth(o, r, z, ok);
        }
    }
    if (o.uncertainty.ptr) {
        float u[EG_RUN];
        egress_load_uncertainty(unc, H, W, frame0, sh, sw, r, u);
        egress_store_uncertainty(o, r, u);
    }
}
// ---- point-cloud egress (include/ppms.h: the formulas).  disparity_egress_kernel's thread mapping, loads and plane stores, plus the two gates
// and the reprojection with q (egress_points' loop, written out in the kernel): a run of points is EG_RUN * C contiguous elements (48 to 128 bytes), which egress_store_run writes
// like any other run.  The upsampled uncertainty is computed once per pixel, where a plane, a gate or w needs it.  Every branch on the struct's
// fields is wave-uniform.
template <class T, int C>
__device__ __forceinline__ void egress_store_points(const ppms_egress_plane& p, const egress_run& r, const float (&X)[EG_RUN], const float (&Y)[EG_RUN],
                                                    const float (&Z)[EG_RUN], const float (&u)[EG_RUN]) {
    T v[EG_RUN * C];
#pragma unroll
    for (int j = 0; j < EG_RUN; ++j) {
        v[j * C] = (T)X[j];
        v[j * C + 1] = (T)Y[j];
        v[j * C + 2] = (T)Z[j];
        if constexpr (C == 4) v[j * C + 3] = (T)u[j];
    }
    egress_store_run<T, C>(p, r.frame, r.y, r.x0, r.n, v);
}
__global__ __launch_bounds__(256) void scene_egress_kernel(const float* __restrict__ flow_up, const float* __restrict__ unc, ppms_egress3d e, int H,
                                                            int W, int frame0, int pad_left, int pad_top, int H0, int W0, float sh, float sw, int rpr,
                                                            int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const ppms_egress& o = e.base;
    const egress_run r = egress_map(idx, rpr, H0, W0, pad_left, pad_top);
    const bool gated = o.depth.ptr || e.points.ptr;                      // a plane the gates act on
    float u[EG_RUN];
    if (o.uncertainty.ptr || (gated && e.max_uncertainty < INFINITY) || (e.points.ptr && e.points_components == 4)) {
        egress_load_uncertainty(unc, H, W, frame0, sh, sw, r, u);
    } else {
#pragma unroll
        for (int j = 0; j < EG_RUN; ++j) u[j] = 0.0f;
    }
    if (o.uncertainty.ptr) egress_store_uncertainty(o, r, u);
    if (!o.disparity.ptr && !gated) return;
    float d[EG_RUN];
    egress_load_disparity(flow_up, H, W, frame0, r, d);
    if (o.disparity.ptr) egress_store_disparity(o, r, d);
    if (o.depth.ptr) {
        const bool gate_z = e.max_depth < INFINITY;
        float z[EG_RUN];
        bool okz[EG_RUN];
#pragma unroll
        for (int j = 0; j < EG_RUN; ++j) {
            const float q = __fdiv_rn(o.fb, d[j]);
            okz[j] = egress_valid(d[j], u[j], o.min_disp, e.max_uncertainty) && (!gate_z || q <= e.max_depth);
            z[j] = okz[j] ? q : INFINITY;
        }
        egress_store_depth(o, r, z, okz);
    }
    if (e.points.ptr) {
        float X[EG_RUN], Y[EG_RUN], Z[EG_RUN];
        // egress_points' loop (egress_shared.h) written out, with the NaN select in it: the same operations in the same order, so the same bits.
        // Through the call, a run at a time, this kernel ran 3 % above the band of the form it had before, and a pixel at a time two samples
        // of six with f32 points lay 0.02 and 0.06 us above it; written out those are inside (docs/LOG_r25.md, section 6: the numbers, and
        // what f16 points show).  The kernel's 72 VGPRs and 7 waves per SIMD (64 and 8 before) are not this loop's, whose text is what it
        // was: the kernel had 66 and 7 with the call too, and what else changed in it is the shared store of a run.
        const bool gate_u = e.max_uncertainty < INFINITY, gate_z = e.max_depth < INFINITY;
        const float yf = (float)r.y;
        float qy[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) qy[i] = e.q[4 * i + 1] * yf;
#pragma unroll
        for (int j = 0; j < EG_RUN; ++j) {
            const bool ok = d[j] >= o.min_disp && (!gate_u || u[j] <= e.max_uncertainty);
            const float xf = (float)(r.x0 + j);
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = ((e.q[4 * i] * xf + qy[i]) + e.q[4 * i + 2] * d[j]) + e.q[4 * i + 3];
            const float pz = __fdiv_rn(v[2], v[3]);
            const bool okp = ok && (!gate_z || (pz > 0.0f && pz <= e.max_depth));
            X[j] = okp ? __fdiv_rn(v[0], v[3]) : __builtin_nanf("");
            Y[j] = okp ? __fdiv_rn(v[1], v[3]) : __builtin_nanf("");
            Z[j] = okp ? pz : __builtin_nanf("");
        }
        if (e.points.format == PPMS_FMT_F32) {
            if (e.points_components == 3) egress_store_points<float, 3>(e.points, r, X, Y, Z, u);
            else egress_store_points<float, 4>(e.points, r, X, Y, Z, u);
        } else {
            if (e.points_components == 3) egress_store_points<_Float16, 3>(e.points, r, X, Y, Z, u);
            else egress_store_points<_Float16, 4>(e.points, r, X, Y, Z, u);
        }
    }
}
extern "C" int ppms_egress_struct_size(void) { return (int)sizeof(ppms_egress); }
extern "C" int ppms_egress3d_struct_size(void) { return (int)sizeof(ppms_egress3d); }
// What both egress entry points check, under the name `who` of the one called: the geometry, the three planes and their constants, and -- from
// ppms_scene_egress (e != nullptr) -- the points plane, q and the gates.  On success the launch geometry (egress_shared.h).
static int egress_check(const char* who, const float* flow_up, const float* unc, int T, int H, int W, int frame0, int n_frames, int pad_left, int pad_top,
                        int H0, int W0, const ppms_egress& o, const ppms_egress3d* e, egress_launch* g) {
    const bool points = e && e->points.ptr;
    if (e)
        PPMS_REQUIRE(o.disparity.ptr || o.depth.ptr || o.uncertainty.ptr || points, "%s: no plane: disparity, depth, uncertainty and points are all NULL", who);
    else
        PPMS_REQUIRE(o.disparity.ptr || o.depth.ptr || o.uncertainty.ptr, "%s: no plane: disparity, depth and uncertainty are all NULL", who);
    if (const int rc = egress_check_geometry(who, T, H, W, frame0, n_frames, pad_left, pad_top, H0, W0, g)) return rc;
    PPMS_REQUIRE(((o.disparity.ptr || o.depth.ptr || points) ? flow_up != nullptr : true) && (o.uncertainty.ptr ? unc != nullptr : true),
                 "%s: null flow_up / unc source of a requested plane", who);
    if (points)
        PPMS_REQUIRE(e->points_components == 3 || e->points_components == 4, "%s: points_components = %d must be 3 or 4", who, e->points_components);
    const struct { const ppms_egress_plane* p; const char *name, *stride; unsigned formats; int comps; } planes[4] = {
        {&o.disparity, "disparity", "disparity.frame_stride", 1u << PPMS_FMT_F32 | 1u << PPMS_FMT_F16 | 1u << PPMS_FMT_U16, 1},
        {&o.depth, "depth", "depth.frame_stride", 1u << PPMS_FMT_F32 | 1u << PPMS_FMT_F16 | 1u << PPMS_FMT_U16, 1},
        {&o.uncertainty, "uncertainty", "uncertainty.frame_stride", 1u << PPMS_FMT_F32 | 1u << PPMS_FMT_U8, 1},
        {points ? &e->points : nullptr, "points", "points.frame_stride", 1u << PPMS_FMT_F32 | 1u << PPMS_FMT_F16, points ? e->points_components : 0}};
    for (const auto& pl : planes) {
        if (!pl.p || !pl.p->ptr) continue;                               // skipped
        const ppms_egress_plane& p = *pl.p;
        PPMS_REQUIRE(p.format >= 0 && p.format <= PPMS_FMT_U8 && (pl.formats >> p.format & 1u),
                     "%s: %s.format = %d is not a format of that plane", who, pl.name, p.format);
        PPMS_REQUIRE(p.reserved == 0, "%s: %s.reserved = %d must be 0", who, pl.name, p.reserved);
        if (const int rc = egress_check_strided(who, pl.name, pl.stride, p.ptr, p.frame_stride, &p.pitch, p.format, n_frames, H0, (int64_t)W0 * pl.comps))
            return rc;
    }
    if (o.depth.ptr) {
        PPMS_REQUIRE(o.fb > 0.0f && o.fb < INFINITY, "%s: a depth plane needs fb = %g > 0", who, (double)o.fb);
        PPMS_REQUIRE(o.depth_scale > 0.0f && o.depth_scale < INFINITY, "%s: a depth plane needs depth_scale = %g > 0", who, (double)o.depth_scale);
        PPMS_REQUIRE(o.min_disp > -INFINITY && o.min_disp < INFINITY, "%s: a depth plane needs a finite min_disp, got %g", who, (double)o.min_disp);
    }
    if (o.disparity.ptr && o.disparity.format == PPMS_FMT_U16)
        PPMS_REQUIRE(o.disp_scale > 0.0f && o.disp_scale < INFINITY, "%s: a u16 disparity needs disp_scale = %g > 0", who, (double)o.disp_scale);
    if (e) {
        PPMS_REQUIRE(e->reserved == 0, "%s: reserved = %d must be 0", who, e->reserved);
        if (const int rc = egress_check_reprojection(who, unc, e->q, o.min_disp, e->max_uncertainty, e->max_depth, points, o.depth.ptr || points,
                                                     e->points_components))
            return rc;
    }
    return PPMS_OK;
}
extern "C" int ppms_disparity_egress(const float* flow_up, const float* unc, int T, int H, int W, int frame0, int n_frames, int pad_left, int pad_top,
                                     int H0, int W0, const ppms_egress* out, void* stream) {
    PPMS_REQUIRE(out, "disparity_egress: null out struct");
    egress_launch g;
    if (const int rc = egress_check("disparity_egress", flow_up, unc, T, H, W, frame0, n_frames, pad_left, pad_top, H0, W0, *out, nullptr, &g)) return rc;
    hipLaunchKernelGGL(disparity_egress_kernel, dim3(ceil_div(g.total, 256)), dim3(256), 0, (hipStream_t)stream, flow_up, unc, *out, H, W, frame0, pad_left,
                       pad_top, H0, W0, g.sh, g.sw, g.rpr, g.total);
    return ppms_check_launch("disparity_egress");
}
extern "C" int ppms_scene_egress(const float* flow_up, const float* unc, int T, int H, int W, int frame0, int n_frames, int pad_left, int pad_top,
                                 int H0, int W0, const ppms_egress3d* out, void* stream) {
    PPMS_REQUIRE(out, "scene_egress: null out struct");
    egress_launch g;
    if (const int rc = egress_check("scene_egress", flow_up, unc, T, H, W, frame0, n_frames, pad_left, pad_top, H0, W0, out->base, out, &g)) return rc;
    hipLaunchKernelGGL(scene_egress_kernel, dim3(ceil_div(g.total, 256)), dim3(256), 0, (hipStream_t)stream, flow_up, unc, *out, H, W, frame0, pad_left,
                       pad_top, H0, W0, g.sh, g.sw, g.rpr, g.total);
    return ppms_check_launch("scene_egress");
}
