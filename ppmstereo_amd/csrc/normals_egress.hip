// Surface-normal egress (ppmstereo_amd/engine.py: disparity_egress with an L.Normals, or an L.Cloud beside a normals plane; driven by output.py's
// OutputSpec(normals=...)): one unit normal per pixel of the cropped plane from the cross stencil over the organised points, and the oriented
// compact cloud whose records carry it (include/ppms.h: the definition, step by step).
//   normals_egress_kernel   the first egress kernel that is not per pixel.  A 256-thread workgroup takes a tile of NT_H x NT_W pixels of ONE frame
//                           -- NT_H rows of NT_W / EG_RUN whole runs -- computes X, Y, Z and the validity of every pixel of the tile and of its
//                           one-pixel rim once (clipped to the crop: a pixel outside it is invalid and nothing is loaded for it), keeps them in
//                           LDS as three float planes and a byte plane, and after ONE barrier every thread forms the stencil of its run from
//                           LDS.  The naive form would reproject 26 pixels per run of 8; this one (NT_H + 2) (NT_W + 2) / (NT_H NT_W) = 1.14 per pixel.
//   cloud_normals_*_kernel  ppms_cloud_egress's count and place launches with one more condition and three more words: a record is kept iff its
//                           point is valid and the first component of the normals plane at its pixel is no NaN; the plane is READ (as the coloured
//                           cloud reads the colour plane), as integers, never recomputed.  A workgroup has CN_WG = 128 threads: its staged records
//                           are up to 28 bytes, and 2048 of them with the indices would not fit 64 KB of static LDS.
// Every operation on a point is one fp32 operation in cloud_points' order (the build contracts nothing), so the points are the organised plane's
// bits.  Every branch on a struct field is wave-uniform, every offset into global memory 64-bit, and no workgroup waits on another.
#include "egress_shared.h"

constexpr int NT_H = 16, NT_W = 16 * EG_RUN;                             // the tile: 16 rows x 128 columns, one run per thread
constexpr int NT_LEFT = 4;                                               // a tile row's column 0 lies at float 4 of its LDS row (a run starts on 16 bytes), the left rim at 3
constexpr int NT_PITCH = NT_LEFT + NT_W + 4;                             // floats per LDS row (136): the right rim at 132
constexpr int NT_ROWS = NT_H + 2, NT_COLS = NT_W + 2;                    // the tile with its rim
constexpr int CN_WG = 128;                                               // threads of an oriented cloud's workgroup
constexpr int CN_PIXELS = CN_WG * EG_RUN;                                // its pixels: the most records it places (1024)

// One pixel's organised point and validity: cloud_points' arithmetic for pixel (y, x) of the cropped plane of output frame `frame`, restated per
// pixel (cloud_points and scene_egress_kernel do not call it: their generated code stays as it is).
__device__ __forceinline__ bool normals_point(const float* __restrict__ flow_up, const float* __restrict__ unc, const ppms_normals& o, bool gate_u,
                                              bool gate_z, int H, int W, int frame0, int64_t frame, int pad_left, int pad_top, float sh, float sw, int y,
                                              int x, float& X, float& Y, float& Z) {
    const int sy = y + pad_top, sx = x + pad_left;
    const float d = fabsf(flow_up[((frame0 + frame) * 2 * H + sy) * W + sx]);                    // channel 0 of (T, 2, H, W)
    bool ok = d >= o.min_disp;                                            // valid_d (false for NaN)
    if (gate_u) {
        const int h = H / 4, w = W / 4;
        const float u = fabsf(bilinear_tap(unc + (frame0 + frame) * h * w, h, w, sh, sw, sy, sx));
        ok = ok && u <= o.max_uncertainty;                                // valid_u (false for NaN)
    }
    const float xf = (float)x, yf = (float)y;
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float qy = o.q[4 * i + 1] * yf;
        v[i] = ((o.q[4 * i] * xf + qy) + o.q[4 * i + 2] * d) + o.q[4 * i + 3];
    }
    X = __fdiv_rn(v[0], v[3]);
    Y = __fdiv_rn(v[1], v[3]);
    Z = __fdiv_rn(v[2], v[3]);
    return ok && (!gate_z || (Z > 0.0f && Z <= o.max_depth));
}
// a run of EG_RUN normals -> the plane: egress_store_points' pattern, restated for 3 components (16 bytes at a time where the run is whole and its
// address 16-byte aligned, element by element otherwise)
template <class T>
__device__ __forceinline__ void normals_store_run(const ppms_egress_plane& p, int64_t frame, int y, int x0, int n, const float (&nrm)[EG_RUN][3]) {
    T v[EG_RUN * 3];
#pragma unroll
    for (int j = 0; j < EG_RUN; ++j) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[j * 3 + c] = (T)nrm[j][c];
    }
    T* dst = (T*)((char*)p.ptr + frame * p.frame_stride + (int64_t)y * p.pitch) + (int64_t)x0 * 3;
    constexpr int BYTES = (int)sizeof(T) * EG_RUN * 3;                   // 48 (f16) or 96 (f32)
    if (n == EG_RUN && ((uintptr_t)dst & 15) == 0) {
        struct chunks { u32x4 q[BYTES / 16]; };
        const chunks c = __builtin_bit_cast(chunks, v);
#pragma unroll
        for (int i = 0; i < BYTES / 16; ++i) gstore16((char*)dst + 16 * i, c.q[i]);
    } else {
#pragma unroll
        for (int j = 0; j < EG_RUN; ++j)
            if (j < n) {
#pragma unroll
                for (int c = 0; c < 3; ++c) dst[j * 3 + c] = v[j * 3 + c];
            }
    }
}
// grid: (tiles of one frame, row-major; n_frames).  tiles_x: tiles per row of tiles.
__global__ __launch_bounds__(256) void normals_egress_kernel(const float* __restrict__ flow_up, const float* __restrict__ unc, ppms_normals o, int H, int W,
                                                              int frame0, int pad_left, int pad_top, int H0, int W0, float sh, float sw, int tiles_x) {
    __shared__ __attribute__((aligned(16))) float sX[NT_ROWS * NT_PITCH], sY[NT_ROWS * NT_PITCH], sZ[NT_ROWS * NT_PITCH];
    __shared__ unsigned char sok[NT_ROWS * NT_PITCH];
    const int64_t frame = blockIdx.y;
    const int ty0 = (int)(blockIdx.x / tiles_x) * NT_H, tx0 = (int)(blockIdx.x % tiles_x) * NT_W;           // the tile's first row and column in the crop
    const bool gate_u = o.max_uncertainty < INFINITY, gate_z = o.max_depth < INFINITY, gate_j = o.max_jump < INFINITY;
    // ---- the tile and its rim: every point once.  Consecutive threads take consecutive x of a row.
    for (int i = threadIdx.x; i < NT_ROWS * NT_COLS; i += 256) {
        const int ry = i / NT_COLS, rc = i % NT_COLS;
        const int y = ty0 - 1 + ry, x = tx0 - 1 + rc, at = ry * NT_PITCH + NT_LEFT - 1 + rc;
        float X = 0.0f, Y = 0.0f, Z = 0.0f;
        bool ok = false;
        if (y >= 0 && y < H0 && x >= 0 && x < W0)                         // a neighbour outside the crop does not exist
            ok = normals_point(flow_up, unc, o, gate_u, gate_z, H, W, frame0, frame, pad_left, pad_top, sh, sw, y, x, X, Y, Z);
        sX[at] = X, sY[at] = Y, sZ[at] = Z, sok[at] = ok ? 1 : 0;
    }
    __syncthreads();
    // ---- the stencil: thread = run (threadIdx.x % 16) of tile row threadIdx.x / 16
    const int y = ty0 + (int)threadIdx.x / (NT_W / EG_RUN), x0 = tx0 + ((int)threadIdx.x % (NT_W / EG_RUN)) * EG_RUN;
    if (y >= H0 || x0 >= W0) return;
    const int n = W0 - x0 < EG_RUN ? W0 - x0 : EG_RUN;
    const int at0 = (y - ty0 + 1) * NT_PITCH + NT_LEFT + (x0 - tx0);
    float nrm[EG_RUN][3];
#pragma unroll
    for (int j = 0; j < EG_RUN; ++j) {                                   // (a pixel past the row's end lies in the tile or its rim: computed, never stored)
        const int at = at0 + j;
        const float CX = sX[at], CY = sY[at], CZ = sZ[at];
        const bool okc = sok[at] != 0;
        const float reach = gate_j ? o.max_jump * fabsf(CZ) : 0.0f;
        // step 1 of the definition: neighbour `nb` is usable
        auto usable = [&](int nb) { return okc && sok[nb] != 0 && (!gate_j || fabsf(sZ[nb] - CZ) <= reach); };
        const int L = at - 1, R = at + 1, U = at - NT_PITCH, D = at + NT_PITCH;
        const bool uL = usable(L), uR = usable(R), uU = usable(U), uD = usable(D);
        // step 2: plus side minus minus side, the centre in place of a side that is not usable
        const float tx[3] = {(uR ? sX[R] : CX) - (uL ? sX[L] : CX), (uR ? sY[R] : CY) - (uL ? sY[L] : CY), (uR ? sZ[R] : CZ) - (uL ? sZ[L] : CZ)};
        const float ty[3] = {(uD ? sX[D] : CX) - (uU ? sX[U] : CX), (uD ? sY[D] : CY) - (uU ? sY[U] : CY), (uD ? sZ[D] : CZ) - (uU ? sZ[U] : CZ)};
        // step 3: n = ty x tx
        float n0 = ty[1] * tx[2] - ty[2] * tx[1];
        float n1 = ty[2] * tx[0] - ty[0] * tx[2];
        float n2 = ty[0] * tx[1] - ty[1] * tx[0];
        // step 4: towards the origin
        const float s = (n0 * CX + n1 * CY) + n2 * CZ;
        if (s > 0.0f) n0 = -n0, n1 = -n1, n2 = -n2;
        // step 5
        const float l = sqrtf((n0 * n0 + n1 * n1) + n2 * n2);
        const bool valid = (uL || uR) && (uU || uD) && l > 0.0f && l < INFINITY;
        nrm[j][0] = valid ? __fdiv_rn(n0, l) : __builtin_nanf("");
        nrm[j][1] = valid ? __fdiv_rn(n1, l) : __builtin_nanf("");
        nrm[j][2] = valid ? __fdiv_rn(n2, l) : __builtin_nanf("");
    }
    if (o.normals.format == PPMS_FMT_F32) normals_store_run<float>(o.normals, frame, y, x0, n, nrm);
    else normals_store_run<_Float16>(o.normals, frame, y, x0, n, nrm);
}
extern "C" int ppms_normals_struct_size(void) { return (int)sizeof(ppms_normals); }
// a normals plane `p` of n_frames x H0 rows of W0 * 3 elements, as both entry points refuse it
static int normals_check_plane(const char* who, const ppms_egress_plane* p, int n_frames, int H0, int W0) {
    PPMS_REQUIRE(p && p->ptr, "%s: null normals plane", who);
    PPMS_REQUIRE(p->format == PPMS_FMT_F32 || p->format == PPMS_FMT_F16, "%s: normals.format = %d is neither PPMS_FMT_F32 nor PPMS_FMT_F16", who, p->format);
    PPMS_REQUIRE(p->reserved == 0, "%s: normals.reserved = %d must be 0", who, p->reserved);
    return egress_check_strided(who, "normals", "normals.frame_stride", p->ptr, p->frame_stride, &p->pitch, p->format, n_frames, H0, (int64_t)W0 * 3);
}
extern "C" int ppms_normals_egress(const float* flow_up, const float* unc, int T, int H, int W, int frame0, int n_frames, int pad_left, int pad_top, int H0,
                                   int W0, const ppms_normals* out, void* stream) {
    const char* who = "normals_egress";
    PPMS_REQUIRE(out, "%s: null out struct", who);
    const ppms_normals& o = *out;
    egress_launch g;
    if (const int rc = egress_check_geometry(who, T, H, W, frame0, n_frames, pad_left, pad_top, H0, W0, &g)) return rc;
    PPMS_REQUIRE(n_frames <= 65535, "%s: n_frames = %d exceeds one grid", who, n_frames);
    PPMS_REQUIRE(flow_up != nullptr, "%s: null flow_up", who);
    if (const int rc = normals_check_plane(who, &o.normals, n_frames, H0, W0)) return rc;
    PPMS_REQUIRE(o.max_jump > 0.0f, "%s: max_jump = %g must be positive (+inf switches the gate off)", who, (double)o.max_jump);       // (false for NaN)
    PPMS_REQUIRE(o.reserved == 0, "%s: reserved = %d must be 0", who, o.reserved);
    if (const int rc = egress_check_reprojection(who, unc, o.q, o.min_disp, o.max_uncertainty, o.max_depth, true, true, 3)) return rc;
    const int64_t tiles_x = (W0 + NT_W - 1) / NT_W, tiles_y = (H0 + NT_H - 1) / NT_H;
    PPMS_REQUIRE(tiles_x * tiles_y <= 0x7fffffff, "%s: %lld tiles exceed one grid", who, (long long)(tiles_x * tiles_y));
    hipLaunchKernelGGL(normals_egress_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)n_frames), dim3(256), 0, (hipStream_t)stream, flow_up, unc, o, H,
                       W, frame0, pad_left, pad_top, H0, W0, g.sh, g.sw, (int)tiles_x);
    return ppms_check_launch("normals_egress");
}
// ------------------------------------------------------------------------------------------------ the oriented compact cloud
// EG_RUN * C words of type Wd from `src`, the first of a run of n pixels: 16-byte loads where the run is whole and its address 16-byte aligned,
// word by word otherwise (past the row's end the last pixel again).  Integers all the way: a colour word may be a signalling NaN's pattern.
template <class Wd, int C>
__device__ __forceinline__ void cloud_load_words(const Wd* src, int n, Wd (&w)[EG_RUN * C]) {
    constexpr int BYTES = (int)sizeof(Wd) * EG_RUN * C;                  // 32 (colour), 48 (f16 normals) or 96 (f32 normals)
    if (n == EG_RUN && ((uintptr_t)src & 15) == 0) {
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
            for (int c = 0; c < C; ++c) w[j * C + c] = gld<Wd>(src + (j < n ? j : n - 1) * C + c);
        }
    }
}
// the run's three words per pixel of the normals plane; returns the mask of the pixels whose normal is valid (the first word is no NaN's pattern)
template <class Wd>
__device__ __forceinline__ unsigned cloud_load_normals(const ppms_egress_plane& p, int64_t frame, const egress_run& r, Wd (&w)[EG_RUN * 3]) {
    const Wd* src = (const Wd*)((const char*)p.ptr + frame * p.frame_stride + (int64_t)r.y * p.pitch) + (int64_t)r.x0 * 3;
    cloud_load_words<Wd, 3>(src, r.n, w);
    constexpr unsigned MAG = sizeof(Wd) == 4 ? 0x7fffffffu : 0x7fffu, INF = sizeof(Wd) == 4 ? 0x7f800000u : 0x7c00u;
    unsigned mask = 0;
#pragma unroll
    for (int j = 0; j < EG_RUN; ++j) mask |= ((unsigned)w[3 * j] & MAG) <= INF ? 1u << j : 0u;
    return mask;
}
// the thread's run, its points and its normals' words: the mask of the pixels whose point AND normal are valid (a thread without a valid point
// loads no normal)
template <class Wd>
__device__ __forceinline__ unsigned cloud_normals_thread(const float* __restrict__ flow_up, const float* __restrict__ unc, const ppms_cloud& c,
                                                         const ppms_egress_plane& normals, int H, int W, int frame0, int pad_left, int pad_top, int H0,
                                                         int W0, float sh, float sw, int rpr, int64_t runs, egress_run& r, float (&X)[EG_RUN],
                                                         float (&Y)[EG_RUN], float (&Z)[EG_RUN], Wd (&w)[EG_RUN * 3]) {
    float u[EG_RUN];
    unsigned mask = cloud_thread<CN_WG>(flow_up, unc, c, false, H, W, frame0, pad_left, pad_top, H0, W0, sh, sw, rpr, runs, r, X, Y, Z, u);
    if (mask) mask &= cloud_load_normals<Wd>(normals, blockIdx.y, r, w);
    return mask;
}
template <class Wd>
__global__ __launch_bounds__(CN_WG) void cloud_normals_count_kernel(const float* __restrict__ flow_up, const float* __restrict__ unc, ppms_cloud c,
                                                                    ppms_egress_plane normals, int H, int W, int frame0, int pad_left, int pad_top, int H0,
                                                                    int W0, float sh, float sw, int rpr, int64_t runs) {
    __shared__ int ws[CN_WG / 64];
    egress_run r = {};
    float X[EG_RUN], Y[EG_RUN], Z[EG_RUN];
    Wd w[EG_RUN * 3];
    const unsigned mask = cloud_normals_thread<Wd>(flow_up, unc, c, normals, H, W, frame0, pad_left, pad_top, H0, W0, sh, sw, rpr, runs, r, X, Y, Z, w);
    const cloud_scan s = cloud_block_scan<CN_WG>(__popc(mask), ws);
    if (threadIdx.x == 0) c.block_counts[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s.total;
}
// cloud_place_kernel's steps with the oriented record: X, Y, Z in T (Wd: the unsigned integer of T's size), [the colour word,] the normal's three
// words.  COLOUR only with T = float.
template <class T, class Wd, bool COLOUR>
__global__ __launch_bounds__(CN_WG) void cloud_normals_place_kernel(const float* __restrict__ flow_up, const float* __restrict__ unc, ppms_cloud c,
                                                                    ppms_egress_plane normals, ppms_egress_plane colour, int H, int W, int frame0,
                                                                    int pad_left, int pad_top, int H0, int W0, float sh, float sw, int rpr, int64_t runs) {
    static_assert(sizeof(T) == sizeof(Wd) && (!COLOUR || sizeof(T) == 4), "words of the record's element size; the colour word is 32 bits");
    constexpr int ES = (int)sizeof(T), RB = ES * (COLOUR ? 7 : 6);      // bytes of a record: 12 (f16), 24 or 28 (f32)
    __shared__ int ws[CN_WG / 64];
    __shared__ __attribute__((aligned(16))) char srec[CN_PIXELS * RB + 16];
    __shared__ __attribute__((aligned(16))) char sidx[CN_PIXELS * 4 + 16];
    const int64_t frame = blockIdx.y;
    // the records in front of this workgroup in its frame
    const int32_t* bc = c.block_counts + frame * gridDim.x;
    int mine = 0;
    for (unsigned i = threadIdx.x; i < blockIdx.x; i += CN_WG) mine += bc[i];
    const int base = cloud_block_scan<CN_WG>(mine, ws).total;
    egress_run r = {};
    float X[EG_RUN], Y[EG_RUN], Z[EG_RUN];
    Wd w[EG_RUN * 3];
    const unsigned mask = cloud_normals_thread<Wd>(flow_up, unc, c, normals, H, W, frame0, pad_left, pad_top, H0, W0, sh, sw, rpr, runs, r, X, Y, Z, w);
    const cloud_scan s = cloud_block_scan<CN_WG>(__popc(mask), ws);
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
        if constexpr (COLOUR)
            cloud_load_words<uint32_t, 1>((const uint32_t*)((const char*)colour.ptr + frame * colour.frame_stride + (int64_t)r.y * colour.pitch) + r.x0, r.n, cw);
        const int pixel = r.y * W0 + r.x0;
#pragma unroll
        for (int j = 0; j < EG_RUN; ++j)
            if (mask >> j & 1u) {
                const int k = s.before + __popc(mask & ((1u << j) - 1u));
                char* rec = srec + shift + k * RB;
                *(T*)(rec) = (T)X[j];
                *(T*)(rec + ES) = (T)Y[j];
                *(T*)(rec + 2 * ES) = (T)Z[j];
                if constexpr (COLOUR) *(uint32_t*)(rec + 12) = cw[j];
#pragma unroll
                for (int i = 0; i < 3; ++i) *(Wd*)(rec + RB - (3 - i) * ES) = w[3 * j + i];
                if (dsti) *(int32_t*)(sidx + shifti + k * 4) = pixel + j;
            }
    }
    __syncthreads();
    cloud_flush<Wd, CN_WG>(srec, dst - shift, shift, shift + n * RB);
    if (dsti) cloud_flush<int32_t, CN_WG>(sidx, dsti - shifti, shifti, shifti + n * 4);
}
extern "C" int64_t ppms_cloud_egress_normals_workspace(int n_frames, int H0, int W0) {
    return n_frames <= 0 ? 0 : n_frames * cloud_blocks_per_frame(H0, W0, CN_WG);
}
extern "C" int ppms_cloud_egress_normals(const float* flow_up, const float* unc, int T, int H, int W, int frame0, int n_frames, int pad_left, int pad_top,
                                         int H0, int W0, const ppms_cloud* out, const ppms_egress_plane* normals, const ppms_egress_plane* colour,
                                         void* stream) {
    const char* who = "cloud_egress_normals";
    egress_launch g;
    int64_t blocks;
    if (const int rc = cloud_check(who, flow_up, unc, T, H, W, frame0, n_frames, pad_left, pad_top, H0, W0, out, CLOUD_NORMALS, g, &blocks, CN_WG)) return rc;
    const ppms_cloud& c = *out;
    if (const int rc = normals_check_plane(who, normals, n_frames, H0, W0)) return rc;
    PPMS_REQUIRE(normals->format == c.format, "%s: normals.format = %d differs from the records' format = %d: a record's elements have one size", who,
                 normals->format, c.format);
    if (c.components == 6) {
        PPMS_REQUIRE(colour == nullptr, "%s: components = 6 (X, Y, Z, nx, ny, nz) takes no colour plane", who);
    } else {
        PPMS_REQUIRE(c.format == PPMS_FMT_F32, "%s: format = %d must be PPMS_FMT_F32 with components = 7: the colour word is the fourth 32-bit word of a record", who,
                     c.format);
        if (const int rc = egress_check_colour_plane(who, "colour", colour, n_frames, H0, W0)) return rc;
    }
    const int64_t runs = (int64_t)H0 * g.rpr;                            // runs of one frame
    const dim3 grid((unsigned)blocks, (unsigned)n_frames), wg(CN_WG);
    hipStream_t s = (hipStream_t)stream;
    const ppms_egress_plane no_colour = {};
#define CN_ARGS flow_up, unc, c, *normals
#define CN_TAIL H, W, frame0, pad_left, pad_top, H0, W0, g.sh, g.sw, g.rpr, runs
    if (c.format == PPMS_FMT_F32) hipLaunchKernelGGL(cloud_normals_count_kernel<uint32_t>, grid, wg, 0, s, CN_ARGS, CN_TAIL);
    else hipLaunchKernelGGL(cloud_normals_count_kernel<uint16_t>, grid, wg, 0, s, CN_ARGS, CN_TAIL);
    if (const int rc = ppms_check_launch("cloud_egress_normals (count)")) return rc;
    if (c.components == 7) hipLaunchKernelGGL((cloud_normals_place_kernel<float, uint32_t, true>), grid, wg, 0, s, CN_ARGS, *colour, CN_TAIL);
    else if (c.format == PPMS_FMT_F32) hipLaunchKernelGGL((cloud_normals_place_kernel<float, uint32_t, false>), grid, wg, 0, s, CN_ARGS, no_colour, CN_TAIL);
    else hipLaunchKernelGGL((cloud_normals_place_kernel<_Float16, uint16_t, false>), grid, wg, 0, s, CN_ARGS, no_colour, CN_TAIL);
#undef CN_ARGS
#undef CN_TAIL
    return ppms_check_launch("cloud_egress_normals (place)");
}
