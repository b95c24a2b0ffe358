// Surface-normal egress (ppmstereo_amd/engine.py: disparity_egress with an L.Normals, or an L.Cloud beside a normals plane; driven by output.py's
// OutputSpec(normals=...)): one unit normal per pixel of the cropped plane from the cross stencil over the organised points (include/ppms.h: the
// definition, step by step).
//   normals_egress_kernel   the first egress kernel that is not per pixel.  A 256-thread workgroup takes a tile of NT_H x NT_W pixels of ONE frame
//                           -- NT_H rows of NT_W / EG_RUN whole runs -- computes X, Y, Z and the validity of every pixel of the tile and of its
//                           one-pixel rim once (clipped to the crop: a pixel outside it is invalid and nothing is loaded for it), keeps them in
//                           LDS as three float planes and a byte plane, and after ONE barrier every thread forms the stencil of its run from
//                           LDS.  The naive form would reproject 26 pixels per run of 8; this one (NT_H + 2) (NT_W + 2) / (NT_H NT_W) = 1.14 per pixel.
// The oriented compact cloud that READS this plane is cloud_egress.hip's.  Every point is egress_points' (egress_shared.h): one fp32 operation
// per step (the build contracts nothing), so the points are the organised plane's bits.  Every branch on a struct field is wave-uniform, every
// offset into global memory 64-bit, and no workgroup waits on another.
#include "egress_shared.h"

constexpr int NT_H = 16, NT_W = 16 * EG_RUN;                             // the tile: 16 rows x 128 columns, one run per thread
constexpr int NT_LEFT = 4;                                               // a tile row's column 0 lies at float 4 of its LDS row (a run starts on 16 bytes), the left rim at 3
constexpr int NT_PITCH = NT_LEFT + NT_W + 4;                             // floats per LDS row (136): the right rim at 132
constexpr int NT_ROWS = NT_H + 2, NT_COLS = NT_W + 2;                    // the tile with its rim

// grid: (tiles of one frame, row-major; n_frames).  tiles_x: tiles per row of tiles.
__global__ __launch_bounds__(256) void normals_egress_kernel(const float* __restrict__ flow_up, const float* __restrict__ unc, ppms_normals o, int H, int W,
                                                              int frame0, int pad_left, int pad_top, int H0, int W0, float sh, float sw, int tiles_x) {
    __shared__ __attribute__((aligned(16))) float sX[NT_ROWS * NT_PITCH], sY[NT_ROWS * NT_PITCH], sZ[NT_ROWS * NT_PITCH];
    __shared__ unsigned char sok[NT_ROWS * NT_PITCH];
    const int64_t frame = blockIdx.y;
    const int ty0 = (int)(blockIdx.x / tiles_x) * NT_H, tx0 = (int)(blockIdx.x % tiles_x) * NT_W;           // the tile's first row and column in the crop
    const bool gate_u = o.max_uncertainty < INFINITY, gate_j = o.max_jump < INFINITY;
    // ---- the tile and its rim: every point once.  Consecutive threads take consecutive x of a row.
    for (int i = threadIdx.x; i < NT_ROWS * NT_COLS; i += 256) {
        const int ry = i / NT_COLS, rc = i % NT_COLS;
        const int y = ty0 - 1 + ry, x = tx0 - 1 + rc, at = ry * NT_PITCH + NT_LEFT - 1 + rc;
        float X = 0.0f, Y = 0.0f, Z = 0.0f;
        bool ok = false;
        if (y >= 0 && y < H0 && x >= 0 && x < W0) {                       // a neighbour outside the crop does not exist
            const int sy = y + pad_top, sx = x + pad_left, h = H / 4, w = W / 4;
            const float d = fabsf(flow_up[((frame0 + frame) * 2 * H + sy) * W + sx]);            // channel 0 of (T, 2, H, W)
            const float u = gate_u ? fabsf(bilinear_tap(unc + (frame0 + frame) * h * w, h, w, sh, sw, sy, sx)) : 0.0f;
            ok = egress_point(o.q, o.min_disp, o.max_uncertainty, o.max_depth, x, y, d, u, X, Y, Z);
        }
        sX[at] = X, sY[at] = Y, sZ[at] = Z, sok[at] = ok ? 1 : 0;
    }
    __syncthreads();
    // ---- the stencil: thread = run (threadIdx.x % 16) of tile row threadIdx.x / 16
    const int y = ty0 + (int)threadIdx.x / (NT_W / EG_RUN), x0 = tx0 + ((int)threadIdx.x % (NT_W / EG_RUN)) * EG_RUN;
    if (y >= H0 || x0 >= W0) return;
    const int n = W0 - x0 < EG_RUN ? W0 - x0 : EG_RUN;
    const int at0 = (y - ty0 + 1) * NT_PITCH + NT_LEFT + (x0 - tx0);
    float nrm[EG_RUN * 3];
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
        nrm[3 * j] = valid ? __fdiv_rn(n0, l) : __builtin_nanf("");
        nrm[3 * j + 1] = valid ? __fdiv_rn(n1, l) : __builtin_nanf("");
        nrm[3 * j + 2] = valid ? __fdiv_rn(n2, l) : __builtin_nanf("");
    }
    if (o.normals.format == PPMS_FMT_F32) {
        egress_store_run<float, 3>(o.normals, frame, y, x0, n, nrm);
    } else {
        _Float16 v[EG_RUN * 3];
#pragma unroll
        for (int i = 0; i < EG_RUN * 3; ++i) v[i] = (_Float16)nrm[i];
        egress_store_run<_Float16, 3>(o.normals, frame, y, x0, n, v);
    }
}
extern "C" int ppms_normals_struct_size(void) { return (int)sizeof(ppms_normals); }
extern "C" int ppms_normals_egress(const float* flow_up, const float* unc, int T, int H, int W, int frame0, int n_frames, int pad_left, int pad_top, int H0,
                                   int W0, const ppms_normals* out, void* stream) {
    const char* who = "normals_egress";
    PPMS_REQUIRE(out, "%s: null out struct", who);
    const ppms_normals& o = *out;
    egress_launch g;
    if (const int rc = egress_check_geometry(who, T, H, W, frame0, n_frames, pad_left, pad_top, H0, W0, &g)) return rc;
    PPMS_REQUIRE(n_frames <= 65535, "%s: n_frames = %d exceeds one grid", who, n_frames);
    PPMS_REQUIRE(flow_up != nullptr, "%s: null flow_up", who);
    if (const int rc = egress_check_normals_plane(who, &o.normals, n_frames, H0, W0)) return rc;
    PPMS_REQUIRE(o.max_jump > 0.0f, "%s: max_jump = %g must be positive (+inf switches the gate off)", who, (double)o.max_jump);       // (false for NaN)
    PPMS_REQUIRE(o.reserved == 0, "%s: reserved = %d must be 0", who, o.reserved);
    if (const int rc = egress_check_reprojection(who, unc, o.q, o.min_disp, o.max_uncertainty, o.max_depth, true, true, 3)) return rc;
    const int64_t tiles_x = (W0 + NT_W - 1) / NT_W, tiles_y = (H0 + NT_H - 1) / NT_H;
    PPMS_REQUIRE(tiles_x * tiles_y <= 0x7fffffff, "%s: %lld tiles exceed one grid", who, (long long)(tiles_x * tiles_y));
    hipLaunchKernelGGL(normals_egress_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)n_frames), dim3(256), 0, (hipStream_t)stream, flow_up, unc, o, H,
                       W, frame0, pad_left, pad_top, H0, W0, g.sh, g.sw, (int)tiles_x);
    return ppms_check_launch("normals_egress");
}
