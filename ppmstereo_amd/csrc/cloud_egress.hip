// Compact point-cloud egress (ppmstereo_amd/engine.py: disparity_egress with an L.Cloud, driven by output.py's OutputSpec(cloud=...)): the valid
// points of ppms_scene_egress's organised points plane, in row-major pixel order, stored densely per frame, with their number and -- where asked --
// their pixel indices (include/ppms.h: the definition).  Two launches on one grid, no atomics and no wait of one workgroup on another:
//   count  every workgroup counts its valid pixels -> block_counts[frame][workgroup]
//   place  every workgroup sums the counts in front of it in its frame (its base), recomputes its points, ranks the valid ones (popcount per
//          thread, a wave64 scan of __shfl_up, a four-wave scan through LDS) and writes record k of its own at base + k.
// The grid is (workgroups per frame, n_frames): a workgroup takes 256 consecutive runs of ONE frame with egress_map's mapping, so thread order is
// row-major pixel order.  Validity and X, Y, Z come from cloud_points in both launches: every operation one fp32 operation in ppms_scene_egress's
// order, so the two launches agree on every pixel and the records carry the organised plane's bits.  (cloud_points, cloud_thread, the scan, the
// flush and cloud_check: egress_shared.h -- normals_egress.hip's oriented cloud is built from the same ones.)
#include "egress_shared.h"

__global__ __launch_bounds__(CLOUD_WG) void cloud_count_kernel(const float* __restrict__ flow_up, const float* __restrict__ unc, ppms_cloud c, int H, int W,
                                                               int frame0, int pad_left, int pad_top, int H0, int W0, float sh, float sw, int rpr,
                                                               int64_t runs) {
    __shared__ int ws[CLOUD_WG / 64];
    egress_run r = {};
    float X[EG_RUN], Y[EG_RUN], Z[EG_RUN], u[EG_RUN];
    const unsigned mask = cloud_thread(flow_up, unc, c, false, H, W, frame0, pad_left, pad_top, H0, W0, sh, sw, rpr, runs, r, X, Y, Z, u);
    const cloud_scan s = cloud_block_scan(__popc(mask), ws);
    if (threadIdx.x == 0) c.block_counts[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s.total;
}
template <class T, int C>
__global__ __launch_bounds__(CLOUD_WG) void cloud_place_kernel(const float* __restrict__ flow_up, const float* __restrict__ unc, ppms_cloud c, int H, int W,
                                                               int frame0, int pad_left, int pad_top, int H0, int W0, float sh, float sw, int rpr,
                                                               int64_t runs) {
    constexpr int RB = (int)sizeof(T) * C;                               // bytes of a record: 6, 8 (f16), 12 or 16 (f32)
    __shared__ int ws[CLOUD_WG / 64];
    __shared__ __attribute__((aligned(16))) char srec[CLOUD_PIXELS * RB + 16];
    __shared__ __attribute__((aligned(16))) char sidx[CLOUD_PIXELS * 4 + 16];
    const int64_t frame = blockIdx.y;
    // the records in front of this workgroup in its frame
    const int32_t* bc = c.block_counts + frame * gridDim.x;
    int mine = 0;
    for (unsigned i = threadIdx.x; i < blockIdx.x; i += CLOUD_WG) mine += bc[i];
    const int base = cloud_block_scan(mine, ws).total;
    egress_run r = {};
    float X[EG_RUN], Y[EG_RUN], Z[EG_RUN], u[EG_RUN];
    const unsigned mask = cloud_thread(flow_up, unc, c, C == 4, H, W, frame0, pad_left, pad_top, H0, W0, sh, sw, rpr, runs, r, X, Y, Z, u);
    const cloud_scan s = cloud_block_scan(__popc(mask), ws);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) c.counts[frame] = base + s.total;
    // this workgroup's records are contiguous in the output: bytes [0, n * RB) from dst.  Staged at the destination's offset inside its 16-byte slot.
    const int64_t room = c.capacity - base;                              // records the frame still takes
    const int n = room <= 0 ? 0 : (s.total < room ? s.total : (int)room);
    if (n == 0) return;                                                  // (uniform over the workgroup)
    char* dst = (char*)c.records + frame * c.frame_stride + (int64_t)base * RB;
    char* dsti = c.index ? (char*)c.index + frame * c.index_frame_stride + (int64_t)base * 4 : nullptr;
    const int shift = (int)((uintptr_t)dst & 15), shifti = (int)((uintptr_t)dsti & 15);
    if (mask) {
        const int pixel = r.y * W0 + r.x0;
#pragma unroll
        for (int j = 0; j < EG_RUN; ++j)
            if (mask >> j & 1u) {
                const int k = s.before + __popc(mask & ((1u << j) - 1u));
                T* rec = (T*)(srec + shift + k * RB);
                rec[0] = (T)X[j];
                rec[1] = (T)Y[j];
                rec[2] = (T)Z[j];
                if constexpr (C == 4) rec[3] = (T)u[j];
                if (dsti) *(int32_t*)(sidx + shifti + k * 4) = pixel + j;
            }
    }
    __syncthreads();
    cloud_flush<T>(srec, dst - shift, shift, shift + n * RB);
    if (dsti) cloud_flush<int32_t>(sidx, dsti - shifti, shifti, shifti + n * 4);
}
// The coloured cloud's place launch (ppms_cloud_egress_colour): cloud_place_kernel<float, 4>'s steps, restated, with the record's fourth word taken
// from the colour plane -- pixel (frame, y, x) of the launch's own n_frames x H0 x W0 crop -- instead of u.  The word is loaded, staged and stored
// as a 32-bit INTEGER (uint32_t / u32x4 all the way: with alpha 255 and a third byte in 0x80..0xBF it is a signalling NaN's pattern, which a
// float move may quieten).  A whole run at a 16-byte aligned address is two 16-byte loads, anything else one aligned 32-bit load per pixel of the
// run.  u is read only where the max_uncertainty gate needs it (want_w = false).  cloud_place_kernel does not call anything new: its code stays.
__global__ __launch_bounds__(CLOUD_WG) void cloud_place_colour_kernel(const float* __restrict__ flow_up, const float* __restrict__ unc, ppms_cloud c,
                                                                      ppms_egress_plane colour, int H, int W, int frame0, int pad_left, int pad_top, int H0,
                                                                      int W0, float sh, float sw, int rpr, int64_t runs) {
    constexpr int RB = 16;                                               // bytes of a record: X, Y, Z (fp32) and the colour word
    __shared__ int ws[CLOUD_WG / 64];
    __shared__ __attribute__((aligned(16))) char srec[CLOUD_PIXELS * RB + 16];
    __shared__ __attribute__((aligned(16))) char sidx[CLOUD_PIXELS * 4 + 16];
    const int64_t frame = blockIdx.y;
    // the records in front of this workgroup in its frame
    const int32_t* bc = c.block_counts + frame * gridDim.x;
    int mine = 0;
    for (unsigned i = threadIdx.x; i < blockIdx.x; i += CLOUD_WG) mine += bc[i];
    const int base = cloud_block_scan(mine, ws).total;
    egress_run r = {};
    float X[EG_RUN], Y[EG_RUN], Z[EG_RUN], u[EG_RUN];
    const unsigned mask = cloud_thread(flow_up, unc, c, false, H, W, frame0, pad_left, pad_top, H0, W0, sh, sw, rpr, runs, r, X, Y, Z, u);
    const cloud_scan s = cloud_block_scan(__popc(mask), ws);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) c.counts[frame] = base + s.total;
    const int64_t room = c.capacity - base;                              // records the frame still takes
    const int n = room <= 0 ? 0 : (s.total < room ? s.total : (int)room);
    if (n == 0) return;                                                  // (uniform over the workgroup)
    char* dst = (char*)c.records + frame * c.frame_stride + (int64_t)base * RB;
    char* dsti = c.index ? (char*)c.index + frame * c.index_frame_stride + (int64_t)base * 4 : nullptr;
    const int shift = (int)((uintptr_t)dst & 15), shifti = (int)((uintptr_t)dsti & 15);
    if (mask) {                                                          // (a thread with a valid pixel has a run: r is its own)
        uint32_t cw[EG_RUN];
        const uint32_t* src = (const uint32_t*)((const char*)colour.ptr + frame * colour.frame_stride + (int64_t)r.y * colour.pitch) + r.x0;
        if (r.n == EG_RUN && ((uintptr_t)src & 15) == 0) {
            const u32x4 a = gld<u32x4>(src), b = gld<u32x4>(src + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cw[j] = a[j];
                cw[4 + j] = b[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < EG_RUN; ++j) cw[j] = gld<uint32_t>(src + (j < r.n ? j : r.n - 1));
        }
        const int pixel = r.y * W0 + r.x0;
#pragma unroll
        for (int j = 0; j < EG_RUN; ++j)
            if (mask >> j & 1u) {
                const int k = s.before + __popc(mask & ((1u << j) - 1u));
                char* rec = srec + shift + k * RB;
                *(float*)(rec) = X[j];
                *(float*)(rec + 4) = Y[j];
                *(float*)(rec + 8) = Z[j];
                *(uint32_t*)(rec + 12) = cw[j];
                if (dsti) *(int32_t*)(sidx + shifti + k * 4) = pixel + j;
            }
    }
    __syncthreads();
    cloud_flush<uint32_t>(srec, dst - shift, shift, shift + n * RB);
    if (dsti) cloud_flush<int32_t>(sidx, dsti - shifti, shifti, shifti + n * 4);
}
extern "C" int ppms_cloud_struct_size(void) { return (int)sizeof(ppms_cloud); }
extern "C" int64_t ppms_cloud_egress_workspace(int n_frames, int H0, int W0) { return n_frames <= 0 ? 0 : n_frames * cloud_blocks_per_frame(H0, W0); }
extern "C" int ppms_cloud_egress(const float* flow_up, const float* unc, int T, int H, int W, int frame0, int n_frames, int pad_left, int pad_top, int H0,
                                 int W0, const ppms_cloud* out, void* stream) {
    egress_launch g;
    int64_t blocks;
    if (const int rc = cloud_check("cloud_egress", flow_up, unc, T, H, W, frame0, n_frames, pad_left, pad_top, H0, W0, out, CLOUD_PLAIN, g, &blocks)) return rc;
    const ppms_cloud& c = *out;
    const int64_t runs = (int64_t)H0 * g.rpr;                            // runs of one frame
    const dim3 grid((unsigned)blocks, (unsigned)n_frames), wg(CLOUD_WG);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cloud_count_kernel, grid, wg, 0, s, flow_up, unc, c, H, W, frame0, pad_left, pad_top, H0, W0, g.sh, g.sw, g.rpr, runs);
    if (const int rc = ppms_check_launch("cloud_egress (count)")) return rc;
#define CLOUD_PLACE(T, C) hipLaunchKernelGGL((cloud_place_kernel<T, C>), grid, wg, 0, s, flow_up, unc, c, H, W, frame0, pad_left, pad_top, H0, W0, g.sh, g.sw, g.rpr, runs)
    if (c.format == PPMS_FMT_F32) {
        if (c.components == 3) CLOUD_PLACE(float, 3);
        else CLOUD_PLACE(float, 4);
    } else {
        if (c.components == 3) CLOUD_PLACE(_Float16, 3);
        else CLOUD_PLACE(_Float16, 4);
    }
#undef CLOUD_PLACE
    return ppms_check_launch("cloud_egress (place)");
}
extern "C" int ppms_cloud_egress_colour(const float* flow_up, const float* unc, int T, int H, int W, int frame0, int n_frames, int pad_left, int pad_top,
                                        int H0, int W0, const ppms_cloud* out, const ppms_egress_plane* colour, void* stream) {
    const char* who = "cloud_egress_colour";
    egress_launch g;
    int64_t blocks;
    if (const int rc = cloud_check(who, flow_up, unc, T, H, W, frame0, n_frames, pad_left, pad_top, H0, W0, out, CLOUD_COLOUR, g, &blocks)) return rc;
    const ppms_cloud& c = *out;
    PPMS_REQUIRE(c.components == 4, "%s: components = %d must be 4: X, Y, Z and the colour word", who, c.components);
    PPMS_REQUIRE(c.format == PPMS_FMT_F32, "%s: format = %d must be PPMS_FMT_F32: the colour word is the fourth 32-bit word of a record", who, c.format);
    if (const int rc = egress_check_colour_plane(who, "colour", colour, n_frames, H0, W0)) return rc;
    const int64_t runs = (int64_t)H0 * g.rpr;                            // runs of one frame
    const dim3 grid((unsigned)blocks, (unsigned)n_frames), wg(CLOUD_WG);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cloud_count_kernel, grid, wg, 0, s, flow_up, unc, c, H, W, frame0, pad_left, pad_top, H0, W0, g.sh, g.sw, g.rpr, runs);
    if (const int rc = ppms_check_launch("cloud_egress_colour (count)")) return rc;
    hipLaunchKernelGGL(cloud_place_colour_kernel, grid, wg, 0, s, flow_up, unc, c, *colour, H, W, frame0, pad_left, pad_top, H0, W0, g.sh, g.sw, g.rpr, runs);
    return ppms_check_launch("cloud_egress_colour (place)");
}
