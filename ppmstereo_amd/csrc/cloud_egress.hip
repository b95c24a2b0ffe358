// Compact point-cloud egress (ppmstereo_amd/engine.py: disparity_egress with an L.Cloud, driven by output.py's OutputSpec(cloud=...)): the valid
// points of ppms_scene_egress's organised points plane, in row-major pixel order, stored densely per frame, with their number and -- where asked --
// their pixel indices (include/ppms.h: the definition).  Two launches on one grid, no atomics and no wait of one workgroup on another:
//   count  every workgroup counts its valid pixels -> block_counts[frame][workgroup]
//   place  every workgroup sums the counts in front of it in its frame (its base), recomputes its points, ranks the valid ones (popcount per
//          thread, a wave64 scan of __shfl_up, a scan of the waves' totals through LDS) and writes record k of its own at base + k.
// The grid is (workgroups per frame, n_frames): a workgroup takes WG consecutive runs of ONE frame with egress_map's mapping, so thread order is
// row-major pixel order.  Validity and X, Y, Z come from egress_points (egress_shared.h) in both launches, so the two agree on every pixel and the
// records carry the organised plane's bits.  ONE kernel pair serves the three entry points; what a record holds behind X, Y, Z is a template
// argument:
//   ppms_cloud_egress          nothing or u
//   ppms_cloud_egress_colour   the colour word: pixel (frame, y, x) of a colour plane of the launch's own n_frames x H0 x W0 crop
//   ppms_cloud_egress_normals  [the colour word,] the three words of a normals plane at the pixel (normals_egress.hip writes it); a record is
//                              kept iff its point is valid AND the plane's first word at its pixel is no NaN
// Both planes are READ, never recomputed, and their words stay INTEGERS from load to store (uint32_t / uint16_t / u32x4 all the way: a colour
// word with alpha 255 and a third byte in 0x80..0xBF is a signalling NaN's pattern, which a float move may quieten).
#include "egress_shared.h"

// threads of a workgroup: 256 for the plain and the coloured cloud (2048 staged records of at most 16 bytes); 128 for the oriented one, whose
// records are up to 28 bytes -- 1024 of them with the indices are what fit 64 KB of static LDS
constexpr int CLOUD_WG = 256, CLOUD_WG_NORMALS = 128;
enum { FOURTH_NONE = 0, FOURTH_U = 1, FOURTH_COLOUR = 2 };               // what follows X, Y, Z in a record (in front of the normal, if any)
template <int BYTES> struct cloud_word { typedef uint32_t type; };      // the unsigned integer of a record element's size
template <> struct cloud_word<2> { typedef uint16_t type; };

// exclusive prefix sum of v over the workgroup's WG threads in thread order, and the workgroup's total: a wave64 scan, then the waves'
// totals through LDS (ws: WG / 64 ints).  Integer sums in a fixed order; ws may be used again after the call.
struct cloud_scan { int before, total; };
template <int WG>
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
template <class E, int WG>
__device__ __forceinline__ void cloud_flush(const char* smem, char* gbase, int lo, int hi) {
    int first = (lo + 15) & ~15, last = hi & ~15;
    if (last < first) first = last = hi;                                 // no whole slot: all of it element by element
    for (int off = first + (int)threadIdx.x * 16; off < last; off += WG * 16) gstore16(gbase + off, *(const u32x4*)(smem + off));
    const int head = (first - lo) / (int)sizeof(E), tail = (hi - last) / (int)sizeof(E);         // fewer than 16 / sizeof(E) elements each
    if ((int)threadIdx.x < head) *(E*)(gbase + lo + threadIdx.x * sizeof(E)) = *(const E*)(smem + lo + threadIdx.x * sizeof(E));
    if ((int)threadIdx.x < tail) *(E*)(gbase + last + threadIdx.x * sizeof(E)) = *(const E*)(smem + last + threadIdx.x * sizeof(E));
}
// EG_RUN * C words of type Wd of plane `p` at the run's pixels: 16-byte loads where the run is whole and its address 16-byte aligned, word by
// word otherwise (past the row's end the last pixel again)
template <class Wd, int C>
__device__ __forceinline__ void cloud_load_words(const ppms_egress_plane& p, int64_t frame, const egress_run& r, Wd (&w)[EG_RUN * C]) {
    const Wd* src = (const Wd*)((const char*)p.ptr + frame * p.frame_stride + (int64_t)r.y * p.pitch) + (int64_t)r.x0 * C;
    constexpr int BYTES = (int)sizeof(Wd) * EG_RUN * C;                  // 32 (colour), 48 (f16 normals) or 96 (f32 normals)
    if (r.n == EG_RUN && ((uintptr_t)src & 15) == 0) {
        struct chunks { u32x4 q[BYTES / 16]; };
        chunks c;
#pragma unroll
        for (int i = 0; i < BYTES / 16; ++i) c.q[i] = gld<u32x4>((const char*)src + 16 * i);
        struct words { Wd w[EG_RUN * C]; };
        const words v = __builtin_bit_cast(words, c);
#pragma unroll
        for (int i = 0; i < EG_RUN * C; ++i) w[i] = v.w[i];
    } else {
#pragma unroll
        for (int j = 0; j < EG_RUN; ++j) {
#pragma unroll
            for (int c = 0; c < C; ++c) w[j * C + c] = gld<Wd>(src + (j < r.n ? j : r.n - 1) * C + c);
        }
    }
}
// What both launches know of a thread: its run r of frame blockIdx.y, d, u (where a gate or `want_u` reads it), X, Y, Z of the run's pixels and,
// with NORMALS, the run's three words per pixel of the normals plane.  Returns the mask of the pixels that make a record, bit j = pixel j of the
// run: the point is valid and, with NORMALS, the normal's first word is no NaN's pattern.  An idle thread past the frame's last run has no pixel,
// and a thread without a valid point loads no normal.
// RESTATED: the points come from egress_points' loop written out here instead of from the call.  The same operations in the same order, so the
// same bits; only the f16 "xyzw" place kernel takes it: through the call that one instantiation ran 0.1 us above the band of the form it had
// before the kernels were merged, and with the loop in place it does not (docs/LOG_r25.md, section 6: the numbers).
template <class Wd, bool NORMALS, int WG, bool RESTATED = false>
__device__ __forceinline__ unsigned cloud_thread(const float* __restrict__ flow_up, const float* __restrict__ unc, const ppms_cloud& c,
                                                 const ppms_egress_plane& normals, bool want_u, int H, int W, int frame0, int pad_left, int pad_top, int H0,
                                                 int W0, float sh, float sw, int rpr, int64_t runs, egress_run& r, float (&X)[EG_RUN], float (&Y)[EG_RUN],
                                                 float (&Z)[EG_RUN], float (&u)[EG_RUN], Wd (&w)[EG_RUN * 3]) {
    const int64_t ridx = (int64_t)blockIdx.x * WG + threadIdx.x;         // the run's number inside the frame
    if (ridx >= runs) return 0u;
    r = egress_map((int64_t)blockIdx.y * runs + ridx, rpr, H0, W0, pad_left, pad_top);
    if (c.max_uncertainty < INFINITY || want_u) {
        egress_load_uncertainty(unc, H, W, frame0, sh, sw, r, u);
    } else {
#pragma unroll
        for (int j = 0; j < EG_RUN; ++j) u[j] = 0.0f;
    }
    float d[EG_RUN];
    egress_load_disparity(flow_up, H, W, frame0, r, d);
    unsigned mask = 0;
    if constexpr (RESTATED) {
        const bool gate_u = c.max_uncertainty < INFINITY, gate_z = c.max_depth < INFINITY;
        const float yf = (float)r.y;
        float qy[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) qy[i] = c.q[4 * i + 1] * yf;
#pragma unroll
        for (int j = 0; j < EG_RUN; ++j) {
            const bool ok = d[j] >= c.min_disp && (!gate_u || u[j] <= c.max_uncertainty);
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
    } else {
        mask = egress_points<EG_RUN>(c.q, c.min_disp, c.max_uncertainty, c.max_depth, r.x0, r.y, r.n, d, u, X, Y, Z);
    }
    if constexpr (NORMALS) {
        if (mask) {
            cloud_load_words<Wd, 3>(normals, blockIdx.y, r, w);
            constexpr unsigned MAG = sizeof(Wd) == 4 ? 0x7fffffffu : 0x7fffu, INF = sizeof(Wd) == 4 ? 0x7f800000u : 0x7c00u;
            unsigned finite = 0;
#pragma unroll
            for (int j = 0; j < EG_RUN; ++j) finite |= ((unsigned)w[3 * j] & MAG) <= INF ? 1u << j : 0u;
            mask &= finite;
        }
    }
    return mask;
}
// T: the record's element, which with NORMALS is the size of the plane's words (a fourth component decides nothing: the count has no such argument)
template <class T, bool NORMALS, int WG>
__global__ __launch_bounds__(WG) void cloud_count_kernel(const float* __restrict__ flow_up, const float* __restrict__ unc, ppms_cloud c, int H, int W,
                                                         int frame0, int pad_left, int pad_top, int H0, int W0, float sh, float sw, int rpr, int64_t runs,
                                                         ppms_egress_plane normals) {
    typedef typename cloud_word<sizeof(T)>::type Wd;
    __shared__ int ws[WG / 64];
    egress_run r = {};
    float X[EG_RUN], Y[EG_RUN], Z[EG_RUN], u[EG_RUN];
    Wd w[EG_RUN * 3];
    const unsigned mask = cloud_thread<Wd, NORMALS, WG>(flow_up, unc, c, normals, false, H, W, frame0, pad_left, pad_top, H0, W0, sh, sw, rpr, runs, r, X, Y, Z, u, w);
    const cloud_scan s = cloud_block_scan<WG>(__popc(mask), ws);
    if (threadIdx.x == 0) c.block_counts[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s.total;
}
// A record: X, Y, Z in T, [u in T | the colour word,] [the normal's three words].  FOURTH_COLOUR only with T = float: the colour word is the
// fourth 32-bit word of a record.
template <class T, int FOURTH, bool NORMALS, int WG>
__global__ __launch_bounds__(WG) void cloud_place_kernel(const float* __restrict__ flow_up, const float* __restrict__ unc, ppms_cloud c, int H, int W,
                                                         int frame0, int pad_left, int pad_top, int H0, int W0, float sh, float sw, int rpr, int64_t runs,
                                                         ppms_egress_plane normals, ppms_egress_plane colour) {
    static_assert(FOURTH != FOURTH_COLOUR || sizeof(T) == 4, "the colour word is 32 bits");
    typedef typename cloud_word<sizeof(T)>::type Wd;
    constexpr int ES = (int)sizeof(T), RB = ES * (3 + (FOURTH != FOURTH_NONE) + 3 * NORMALS);   // bytes of a record: 6 .. 16, oriented 12 .. 28
    constexpr int PIXELS = WG * EG_RUN;                                  // pixels of a workgroup: the most records it places
    __shared__ int ws[WG / 64];
    __shared__ __attribute__((aligned(16))) char srec[PIXELS * RB + 16];
    __shared__ __attribute__((aligned(16))) char sidx[PIXELS * 4 + 16];
    const int64_t frame = blockIdx.y;
    // the records in front of this workgroup in its frame
    const int32_t* bc = c.block_counts + frame * gridDim.x;
    int mine = 0;
    for (unsigned i = threadIdx.x; i < blockIdx.x; i += WG) mine += bc[i];
    const int base = cloud_block_scan<WG>(mine, ws).total;
    egress_run r = {};
    float X[EG_RUN], Y[EG_RUN], Z[EG_RUN], u[EG_RUN];
    Wd w[EG_RUN * 3];
    constexpr bool RESTATED = sizeof(T) == 2 && FOURTH == FOURTH_U && !NORMALS;          // the f16 "xyzw" cloud (cloud_thread: why)
    const unsigned mask = cloud_thread<Wd, NORMALS, WG, RESTATED>(flow_up, unc, c, normals, FOURTH == FOURTH_U, H, W, frame0, pad_left, pad_top, H0, W0, sh, sw, rpr, runs, r,
                                                        X, Y, Z, u, w);
    const cloud_scan s = cloud_block_scan<WG>(__popc(mask), ws);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) c.counts[frame] = base + s.total;
    // this workgroup's records are contiguous in the output: bytes [0, n * RB) from dst.  Staged at the destination's offset inside its 16-byte slot.
    const int64_t room = c.capacity - base;                              // records the frame still takes
    const int n = room <= 0 ? 0 : (s.total < room ? s.total : (int)room);
    if (n == 0) return;                                                  // (uniform over the workgroup)
    char* dst = (char*)c.records + frame * c.frame_stride + (int64_t)base * RB;
    char* dsti = c.index ? (char*)c.index + frame * c.index_frame_stride + (int64_t)base * 4 : nullptr;
    const int shift = (int)((uintptr_t)dst & 15), shifti = (int)((uintptr_t)dsti & 15);
    if (mask) {                                                          // (a thread with a valid pixel has a run: r is its own)
        uint32_t cw[EG_RUN] = {};
        if constexpr (FOURTH == FOURTH_COLOUR) cloud_load_words<uint32_t, 1>(colour, frame, r, cw);
        const int pixel = r.y * W0 + r.x0;
#pragma unroll
        for (int j = 0; j < EG_RUN; ++j)
            if (mask >> j & 1u) {
                const int k = s.before + __popc(mask & ((1u << j) - 1u));
                char* rec = srec + shift + k * RB;
                *(T*)(rec) = (T)X[j];
                *(T*)(rec + ES) = (T)Y[j];
                *(T*)(rec + 2 * ES) = (T)Z[j];
                if constexpr (FOURTH == FOURTH_U) *(T*)(rec + 3 * ES) = (T)u[j];
                if constexpr (FOURTH == FOURTH_COLOUR) *(uint32_t*)(rec + 12) = cw[j];
                if constexpr (NORMALS) {
#pragma unroll
                    for (int i = 0; i < 3; ++i) *(Wd*)(rec + RB - (3 - i) * ES) = w[3 * j + i];
                }
                if (dsti) *(int32_t*)(sidx + shifti + k * 4) = pixel + j;
            }
    }
    __syncthreads();
    cloud_flush<Wd, WG>(srec, dst - shift, shift, shift + n * RB);
    if (dsti) cloud_flush<int32_t, WG>(sidx, dsti - shifti, shifti, shifti + n * 4);
}
// workgroups of `wg` threads per frame; 0 for a geometry the entry points refuse
static inline int64_t cloud_blocks_per_frame(int H0, int W0, int wg) {
    if (H0 <= 0 || W0 <= 0 || (int64_t)H0 * W0 > 0x7fffffff) return 0;
    return ((int64_t)H0 * ((W0 + EG_RUN - 1) / EG_RUN) + wg - 1) / wg;
}
// ---- host: what the three entry points check alike, under the name `who` of the one called; on success the launch geometry and the workgroups
// per frame.  layout: what a record holds beside X, Y, Z -- CLOUD_PLAIN (ppms_cloud_egress: 3 or 4 components, the fourth u), CLOUD_COLOUR
// (ppms_cloud_egress_colour: the fourth component is the colour word, so nothing but the max_uncertainty gate reads unc), CLOUD_NORMALS
// (ppms_cloud_egress_normals: 6 or 7 components, workgroups of CLOUD_WG_NORMALS threads; unc as for CLOUD_COLOUR)
enum { CLOUD_PLAIN = 0, CLOUD_COLOUR = 1, CLOUD_NORMALS = 2 };
static int cloud_check(const char* who, const float* flow_up, const float* unc, int T, int H, int W, int frame0, int n_frames, int pad_left, int pad_top,
                       int H0, int W0, const ppms_cloud* out, int layout, egress_launch& g, int64_t* blocks_out) {
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
    const int64_t blocks = cloud_blocks_per_frame(H0, W0, layout == CLOUD_NORMALS ? CLOUD_WG_NORMALS : CLOUD_WG);
    PPMS_REQUIRE(c.block_counts != nullptr && c.block_counts_len >= n_frames * blocks,
                 "%s: block_counts is null or block_counts_len = %lld is less than the %lld entries of %s", who,
                 (long long)c.block_counts_len, (long long)(n_frames * blocks),
                 layout == CLOUD_NORMALS ? "ppms_cloud_egress_normals_workspace" : "ppms_cloud_egress_workspace");
    *blocks_out = blocks;
    return egress_check_reprojection(who, unc, c.q, c.min_disp, c.max_uncertainty, c.max_depth, true, true, layout == CLOUD_PLAIN ? c.components : 3);
}
// ---- host: the one launcher behind the three entry points: cloud_check, what the layout requires beyond it, the grid, count, place
static int cloud_launch(const char* who, int layout, const float* flow_up, const float* unc, int T, int H, int W, int frame0, int n_frames, int pad_left,
                        int pad_top, int H0, int W0, const ppms_cloud* out, const ppms_egress_plane* colour, const ppms_egress_plane* normals, void* stream) {
    egress_launch g;
    int64_t blocks;
    if (const int rc = cloud_check(who, flow_up, unc, T, H, W, frame0, n_frames, pad_left, pad_top, H0, W0, out, layout, g, &blocks)) return rc;
    const ppms_cloud& c = *out;
    const bool f32 = c.format == PPMS_FMT_F32;
    if (layout == CLOUD_COLOUR) {
        PPMS_REQUIRE(c.components == 4, "%s: components = %d must be 4: X, Y, Z and the colour word", who, c.components);
        PPMS_REQUIRE(f32, "%s: format = %d must be PPMS_FMT_F32: the colour word is the fourth 32-bit word of a record", who, c.format);
        if (const int rc = egress_check_colour_plane(who, "colour", colour, n_frames, H0, W0)) return rc;
    } else if (layout == CLOUD_NORMALS) {
        if (const int rc = egress_check_normals_plane(who, normals, n_frames, H0, W0)) return rc;
        PPMS_REQUIRE(normals->format == c.format, "%s: normals.format = %d differs from the records' format = %d: a record's elements have one size", who,
                     normals->format, c.format);
        if (c.components == 6) {
            PPMS_REQUIRE(colour == nullptr, "%s: components = 6 (X, Y, Z, nx, ny, nz) takes no colour plane", who);
        } else {
            PPMS_REQUIRE(f32, "%s: format = %d must be PPMS_FMT_F32 with components = 7: the colour word is the fourth 32-bit word of a record", who, c.format);
            if (const int rc = egress_check_colour_plane(who, "colour", colour, n_frames, H0, W0)) return rc;
        }
    }
    const int64_t runs = (int64_t)H0 * g.rpr;                            // runs of one frame
    const dim3 grid((unsigned)blocks, (unsigned)n_frames), wg(layout == CLOUD_NORMALS ? CLOUD_WG_NORMALS : CLOUD_WG);
    const ppms_egress_plane none = {}, pn = normals ? *normals : none, pc = colour ? *colour : none;
    char what[64];
#define CLOUD_ARGS grid, wg, 0, (hipStream_t)stream, flow_up, unc, c, H, W, frame0, pad_left, pad_top, H0, W0, g.sh, g.sw, g.rpr, runs, pn
#define CLOUD_COUNT(T, NORMALS, WG) hipLaunchKernelGGL((cloud_count_kernel<T, NORMALS, WG>), CLOUD_ARGS)
#define CLOUD_PLACE(T, FOURTH, NORMALS, WG) hipLaunchKernelGGL((cloud_place_kernel<T, FOURTH, NORMALS, WG>), CLOUD_ARGS, pc)
    if (layout != CLOUD_NORMALS) CLOUD_COUNT(float, false, CLOUD_WG);
    else if (f32) CLOUD_COUNT(float, true, CLOUD_WG_NORMALS);
    else CLOUD_COUNT(_Float16, true, CLOUD_WG_NORMALS);
    snprintf(what, sizeof(what), "%s (count)", who);
    if (const int rc = ppms_check_launch(what)) return rc;
    if (layout == CLOUD_NORMALS) {
        if (c.components == 7) CLOUD_PLACE(float, FOURTH_COLOUR, true, CLOUD_WG_NORMALS);
        else if (f32) CLOUD_PLACE(float, FOURTH_NONE, true, CLOUD_WG_NORMALS);
        else CLOUD_PLACE(_Float16, FOURTH_NONE, true, CLOUD_WG_NORMALS);
    } else if (layout == CLOUD_COLOUR) {
        CLOUD_PLACE(float, FOURTH_COLOUR, false, CLOUD_WG);
    } else if (f32) {
        if (c.components == 3) CLOUD_PLACE(float, FOURTH_NONE, false, CLOUD_WG);
        else CLOUD_PLACE(float, FOURTH_U, false, CLOUD_WG);
    } else {
        if (c.components == 3) CLOUD_PLACE(_Float16, FOURTH_NONE, false, CLOUD_WG);
        else CLOUD_PLACE(_Float16, FOURTH_U, false, CLOUD_WG);
    }
#undef CLOUD_ARGS
#undef CLOUD_COUNT
#undef CLOUD_PLACE
    snprintf(what, sizeof(what), "%s (place)", who);
    return ppms_check_launch(what);
}
extern "C" int ppms_cloud_struct_size(void) { return (int)sizeof(ppms_cloud); }
extern "C" int64_t ppms_cloud_egress_workspace(int n_frames, int H0, int W0) { return n_frames <= 0 ? 0 : n_frames * cloud_blocks_per_frame(H0, W0, CLOUD_WG); }
extern "C" int64_t ppms_cloud_egress_normals_workspace(int n_frames, int H0, int W0) {
    return n_frames <= 0 ? 0 : n_frames * cloud_blocks_per_frame(H0, W0, CLOUD_WG_NORMALS);
}
extern "C" int ppms_cloud_egress(const float* flow_up, const float* unc, int T, int H, int W, int frame0, int n_frames, int pad_left, int pad_top, int H0,
                                 int W0, const ppms_cloud* out, void* stream) {
    return cloud_launch("cloud_egress", CLOUD_PLAIN, flow_up, unc, T, H, W, frame0, n_frames, pad_left, pad_top, H0, W0, out, nullptr, nullptr, stream);
}
extern "C" int ppms_cloud_egress_colour(const float* flow_up, const float* unc, int T, int H, int W, int frame0, int n_frames, int pad_left, int pad_top,
                                        int H0, int W0, const ppms_cloud* out, const ppms_egress_plane* colour, void* stream) {
    return cloud_launch("cloud_egress_colour", CLOUD_COLOUR, flow_up, unc, T, H, W, frame0, n_frames, pad_left, pad_top, H0, W0, out, colour, nullptr, stream);
}
extern "C" int ppms_cloud_egress_normals(const float* flow_up, const float* unc, int T, int H, int W, int frame0, int n_frames, int pad_left, int pad_top,
                                         int H0, int W0, const ppms_cloud* out, const ppms_egress_plane* normals, const ppms_egress_plane* colour,
                                         void* stream) {
    return cloud_launch("cloud_egress_normals", CLOUD_NORMALS, flow_up, unc, T, H, W, frame0, n_frames, pad_left, pad_top, H0, W0, out, colour, normals, stream);
}
