// HBM-bound helper kernels that an iteration of ScaleEngine launches (ppmstereo_amd/engine.py): depthwise conv + GELU, flow im2col,
// uncertainty tail, tap gather-sum, flow += delta_flow and the convex upsampling (also called from ppmstereo_amd/ppmstereo.py).
#include "common.h"

// ------------------------------------------------------------------------------------------------ depthwise conv
// y = gelu(x + dw_k(x) + b), PCBlock4_Deep_nopool_res.forward (ppmtereo_update.py:1026-1027)
// one thread = a run of DW_PX pixels along x times 8 channels: per kernel row it loads the DW_PX + K - 1 window
// positions once (16-byte loads of the hi and lo planes, channel-last rows are contiguous) and sweeps the K taps over
// them from registers; the weights sit in LDS transposed to [tap][channel] (two b128 reads per tap).
constexpr int DW_PX = 2;            // (4: 31.6 us at the 1/4 scale, 2: 28.3 -- twice the threads hide more of the load latency)
template <int K>
__global__ __launch_bounds__(256) void dwconv_gelu_kernel(ppms_sp x, ppms_sp y, const float* __restrict__ w, const float* __restrict__ b,
                                                          int H, int W, int64_t rows, int groups) {
    __shared__ __attribute__((aligned(16))) float wl[K * K * 64];
    const int C = groups * 8;
    for (int i = threadIdx.x; i < K * K * C; i += 256) {
        const int c = i % C, tap = i / C;
        wl[tap * C + c] = w[c * K * K + tap];
    }
    __syncthreads();
    const int rpr = (W + DW_PX - 1) / DW_PX;                       // runs per image row
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * rpr * groups) return;
    const int c0 = (int)(idx % groups) * 8;
    const int64_t run = idx / groups;
    const int px0 = (int)(run % rpr) * DW_PX;
    const int64_t row = run / rpr;                                 // frame * H + y
    const int py = (int)(row % H);
    const int64_t pix0 = row * W + px0;
    const bf16_t* xh = (const bf16_t*)x.hi + c0;
    const bf16_t* xl = (const bf16_t*)x.lo + c0;
    float acc[DW_PX][8], x0[DW_PX][8];
    {
        const f32x4 b0 = *(const f32x4*)(b + c0), b1 = *(const f32x4*)(b + c0 + 4);
#pragma unroll
        for (int p = 0; p < DW_PX; ++p)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                acc[p][j] = j < 4 ? b0[j & 3] : b1[j & 3];
                x0[p][j] = 0.0f;
            }
    }
    constexpr int R = K / 2, NW = DW_PX + K - 1;
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
        const int yy = py + ky - R;
        if ((unsigned)yy >= (unsigned)H) continue;
        float win[NW][8];
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int xx = px0 - R + i;
            bf16x8 h8 = {0, 0, 0, 0, 0, 0, 0, 0}, l8 = {0, 0, 0, 0, 0, 0, 0, 0};
            if ((unsigned)xx < (unsigned)W) {
                const int64_t q = pix0 + (int64_t)(ky - R) * W + (i - R);
                h8 = *(const bf16x8*)(xh + q * x.ld);
                l8 = *(const bf16x8*)(xl + q * x.ld);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) win[i][j] = join_bf16(h8[j], l8[j]);
        }
        if (ky == R) {
#pragma unroll
            for (int p = 0; p < DW_PX; ++p)
#pragma unroll
                for (int j = 0; j < 8; ++j) x0[p][j] = win[p + R][j];
        }
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            const f32x4 w0 = *(const f32x4*)(wl + (ky * K + kx) * C + c0), w1 = *(const f32x4*)(wl + (ky * K + kx) * C + c0 + 4);
#pragma unroll
            for (int p = 0; p < DW_PX; ++p)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[p][j] += (j < 4 ? w0[j & 3] : w1[j & 3]) * win[p + kx][j];   // out-of-image taps add 0 * w
        }
    }
#pragma unroll
    for (int p = 0; p < DW_PX; ++p) {
        if (px0 + p >= W) break;
        bf16x8 oh, ol;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            bf16_t hi, lo;
            split_bf16(gelu_erf(x0[p][j] + acc[p][j]), hi, lo);
            oh[j] = hi;
            ol[j] = lo;
        }
        *(bf16x8*)((bf16_t*)y.hi + (pix0 + p) * y.ld + c0) = oh;
        *(bf16x8*)((bf16_t*)y.lo + (pix0 + p) * y.ld + c0) = ol;
    }
}

extern "C" int ppms_dwconv_gelu(ppms_sp x, ppms_sp y, const float* w, const float* b, int k, int BT, int H, int W, void* stream) {
    PPMS_REQUIRE(k == 1 || k == 7, "dwconv_gelu: k=%d (only 1 and 7)", k);
    PPMS_REQUIRE(x.hi && x.lo && y.hi && y.lo && x.c == y.c && x.c > 0 && x.c <= 64 && x.c % 8 == 0 && x.ld % 8 == 0 && y.ld % 8 == 0,
                 "dwconv_gelu: views must have c <= 64 and c, ld multiples of 8");
    // the kernel loads the planes 16 bytes (8 channels) and the bias 16 bytes (4 floats) at a time
    PPMS_REQUIRE((((uintptr_t)x.hi | (uintptr_t)x.lo | (uintptr_t)y.hi | (uintptr_t)y.lo) & 15) == 0,
                 "dwconv_gelu: the planes of x and y must be 16-byte aligned (a view starts at a multiple of 8 channels)");
    PPMS_REQUIRE(w != nullptr && b != nullptr && ((uintptr_t)b & 15) == 0, "dwconv_gelu: w and a 16-byte aligned bias expected");
    PPMS_REQUIRE(BT > 0 && H > 0 && W > 0, "dwconv_gelu: bad shape BT=%d H=%d W=%d", BT, H, W);
    const int64_t rows = (int64_t)BT * H;
    const int groups = x.c / 8;
    const dim3 grid(ceil_div(rows * ((W + DW_PX - 1) / DW_PX) * groups, 256));
    if (k == 1)
        hipLaunchKernelGGL(dwconv_gelu_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, y, w, b, H, W, rows, groups);
    else
        hipLaunchKernelGGL(dwconv_gelu_kernel<7>, grid, dim3(256), 0, (hipStream_t)stream, x, y, w, b, H, W, rows, groups);
    return ppms_check_launch("dwconv_gelu");
}

// ------------------------------------------------------------------------------------------------ flow im2col (convf1 7x7, Cin=2)
__global__ __launch_bounds__(256) void flow_patch7_kernel(const float* __restrict__ flow, ppms_sp patch, int H, int W, int64_t P) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= P * 128) return;
    const int k = (int)(idx & 127);
    const int64_t pix = idx >> 7;
    float v = 0.0f;
    if (k < 98) {
        const int tap = k >> 1, c = k & 1;
        const int ky = tap / 7, kx = tap - ky * 7;
        const int px = (int)(pix % W), py = (int)((pix / W) % H);
        const int xx = px + kx - 3, yy = py + ky - 3;
        if ((unsigned)xx < (unsigned)W && (unsigned)yy < (unsigned)H) v = flow[(pix + (int64_t)(ky - 3) * W + (kx - 3)) * 2 + c];
    }
    bf16_t hi, lo;
    split_bf16(v, hi, lo);
    ((bf16_t*)patch.hi)[pix * patch.ld + k] = hi;
    ((bf16_t*)patch.lo)[pix * patch.ld + k] = lo;
}

extern "C" int ppms_flow_patch7(const float* flow_nhwc, ppms_sp patch, int BT, int H, int W, void* stream) {
    PPMS_REQUIRE(flow_nhwc && patch.hi && patch.lo && patch.ld >= 128, "flow_patch7: bad arguments");
    const int64_t P = (int64_t)BT * H * W;
    hipLaunchKernelGGL(flow_patch7_kernel, dim3(ceil_div(P * 128, 256)), dim3(256), 0, (hipStream_t)stream, flow_nhwc, patch, H, W, P);
    return ppms_check_launch("flow_patch7");
}

// ------------------------------------------------------------------------------------------------ uncertainty tail
// unc = sigmoid(w . x + b) (128 -> 1), plus deterministic per-(frame, 256-pixel block) partial sums
__global__ __launch_bounds__(256) void unc_tail_kernel(ppms_sp x, const float* __restrict__ w, float bias, float* __restrict__ unc,
                                                       float* __restrict__ partial, int HW, int nblk) {
    __shared__ float red[16];
    const int frame = blockIdx.y, blk = blockIdx.x;
    const int sub = threadIdx.x & 15, grp = threadIdx.x >> 4;   // 16 lanes per pixel, 8 channels each
    float wv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) wv[j] = w[sub * 8 + j];
    // all 16 pixels of a lane group are requested before the first is consumed (the loop used to wait out one memory round trip per pixel:
    // 16 us per launch at every scale); the sums keep their order (per pixel: lanes by shuffle; per block: pixel order), so the
    // confidences are the same bits as before
    bf16x8 h8[16], l8[16];
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        const int pin = blk * 256 + it * 16 + grp;
        const int64_t pix = (int64_t)frame * HW + (pin < HW ? pin : HW - 1);
        h8[it] = gld<bf16x8>((const bf16_t*)x.hi + pix * x.ld + sub * 8);
        l8[it] = gld<bf16x8>((const bf16_t*)x.lo + pix * x.ld + sub * 8);
    }
    float local = 0.0f;
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        const int pin = blk * 256 + it * 16 + grp;
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += wv[j] * join_bf16(h8[it][j], l8[it][j]);
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        s += __shfl_xor(s, 8);
        if (pin < HW && sub == 0) {
            const float u = sigmoid_f(s + bias);
            unc[(int64_t)frame * HW + pin] = u;
            local += u;
        }
    }
    // fixed-order block sum: 16 group leaders -> LDS -> thread 0
    if (sub == 0) red[grp] = local;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.0f;
        for (int i = 0; i < 16; ++i) t += red[i];
        partial[frame * nblk + blk] = t;
    }
}

extern "C" int ppms_unc_tail(ppms_sp x, const float* w, float bias, float* unc, float* partial, int BT, int HW, void* stream) {
    PPMS_REQUIRE(x.hi && x.lo && x.c == 128 && x.ld % 8 == 0, "unc_tail: expects a 128-channel SP view");
    const int nblk = ceil_div(HW, 256);
    hipLaunchKernelGGL(unc_tail_kernel, dim3(nblk, BT), dim3(256), 0, (hipStream_t)stream, x, w, bias, unc, partial, HW, nblk);
    return ppms_check_launch("unc_tail");
}

// ------------------------------------------------------------------------------------------------ tap gather-sum
// Tail of a conv with very few output channels computed as a 1x1 GEMM to (taps x cout) channels:
//   out[p][c] = bias[c] + sum_tap y[p + d(tap)][tap*cout + c],  d(tap) = (kz - kt/2, ky - kh/2, kx - kw/2), zero outside.
// Used for FlowHead3D.conv2 (256 -> 2, 3x3x3, ppmtereo_update.py:674): 8 GEMM k-steps instead of 216.
__global__ __launch_bounds__(256) void tap_gather_sum_kernel(const float* __restrict__ y, int y_ld, const float* __restrict__ bias,
                                                             float* __restrict__ out, int out_ld, float* __restrict__ accum, int accum_ld, int cout,
                                                             int kt, int kh, int kw, int T, int H, int W, int t_halo, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % cout);
    const int64_t pix = idx / cout;
    const int x = (int)(pix % W), yy = (int)((pix / W) % H), t = (int)(pix / ((int64_t)W * H));
    float acc = bias ? bias[c] : 0.0f;
    int tap = 0;
    for (int kz = 0; kz < kt; ++kz)
        for (int ky = 0; ky < kh; ++ky)
            for (int kx = 0; kx < kw; ++kx, ++tap) {
                const int tt = t + kz - kt / 2, y2 = yy + ky - kh / 2, x2 = x + kx - kw / 2;
                if ((unsigned)(tt + t_halo) < (unsigned)(T + 2 * t_halo) && (unsigned)y2 < (unsigned)H && (unsigned)x2 < (unsigned)W)
                    acc += y[(((int64_t)tt * H + y2) * W + x2) * y_ld + tap * cout + c];
            }
    out[pix * out_ld + c] = acc;
    if (accum != nullptr) accum[pix * accum_ld + c] += acc;          // flow += delta_flow (ppmstereo.py:571) without a second launch
}
// 3 x 3 x 3 taps (the flow head's tail, 20 launches per clip), fully unrolled: all 27 loads of a thread are in flight together -- the generic
// kernel's runtime loops wait out a memory round trip per tap (12-14 us per launch whatever the map size).  Same order of additions.
__global__ __launch_bounds__(256) void tap_gather_sum333_kernel(const float* __restrict__ y, int y_ld, const float* __restrict__ bias,
                                                                float* __restrict__ out, int out_ld, float* __restrict__ accum, int accum_ld, int cout,
                                                                int T, int H, int W, int t_halo, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % cout);
    const int64_t pix = idx / cout;
    const int x = (int)(pix % W), yy = (int)((pix / W) % H), t = (int)(pix / ((int64_t)W * H));
    float v[27];
#pragma unroll
    for (int tap = 0; tap < 27; ++tap) {
        const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
        const int tt = t + kz - 1, y2 = yy + ky - 1, x2 = x + kx - 1;
        const bool ok = (unsigned)(tt + t_halo) < (unsigned)(T + 2 * t_halo) && (unsigned)y2 < (unsigned)H && (unsigned)x2 < (unsigned)W;
        v[tap] = ok ? y[(((int64_t)tt * H + y2) * W + x2) * y_ld + tap * cout + c] : 0.0f;
    }
    float acc = bias ? bias[c] : 0.0f;
#pragma unroll
    for (int tap = 0; tap < 27; ++tap) {
        const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
        const int tt = t + kz - 1, y2 = yy + ky - 1, x2 = x + kx - 1;
        const bool ok = (unsigned)(tt + t_halo) < (unsigned)(T + 2 * t_halo) && (unsigned)y2 < (unsigned)H && (unsigned)x2 < (unsigned)W;
        if (ok) acc += v[tap];                                     // (skipped, not "+ 0": the generic kernel's sum, bit for bit)
    }
    out[pix * out_ld + c] = acc;
    if (accum != nullptr) accum[pix * accum_ld + c] += acc;
}
// accum (optional, [pixels][accum_ld], accum_ld >= cout): accum[p][c] += out[p][c] in the same launch
extern "C" int ppms_tap_gather_sum(const float* y, int y_ld, const float* bias, float* out, int out_ld, float* accum, int accum_ld, int cout, int kt,
                                   int kh, int kw, int T, int H, int W, int t_halo, void* stream) {
    PPMS_REQUIRE(y && out && cout > 0 && kt * kh * kw * cout <= y_ld && out_ld >= cout && t_halo >= 0, "tap_gather_sum: bad arguments");
    PPMS_REQUIRE(accum == nullptr || accum_ld >= cout, "tap_gather_sum: accum_ld=%d < cout=%d", accum_ld, cout);
    const int64_t total = (int64_t)T * H * W * cout;
    if (kt == 3 && kh == 3 && kw == 3)
        hipLaunchKernelGGL(tap_gather_sum333_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, y, y_ld, bias, out, out_ld, accum,
                           accum_ld, cout, T, H, W, t_halo, total);
    else
        hipLaunchKernelGGL(tap_gather_sum_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, y, y_ld, bias, out, out_ld, accum, accum_ld,
                           cout, kt, kh, kw, T, H, W, t_halo, total);
    return ppms_check_launch("tap_gather_sum");
}

// ------------------------------------------------------------------------------------------------ flow += delta_flow
__global__ __launch_bounds__(256) void flow_add_kernel(float* __restrict__ flow, const float* __restrict__ dflow, int dflow_ld, int64_t P) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= P * 2) return;
    flow[idx] += dflow[(idx >> 1) * dflow_ld + (idx & 1)];
}
extern "C" int ppms_flow_add(float* flow_nhwc, const float* dflow, int dflow_ld, int64_t pixels, void* stream) {
    PPMS_REQUIRE(flow_nhwc && dflow && dflow_ld >= 2, "flow_add: bad arguments");
    hipLaunchKernelGGL(flow_add_kernel, dim3(ceil_div(pixels * 2, 256)), dim3(256), 0, (hipStream_t)stream, flow_nhwc, dflow, dflow_ld, pixels);
    return ppms_check_launch("flow_add");
}

// ------------------------------------------------------------------------------------------------ convex upsample
// out[n,c,4y+i,4x+j] = sum_k softmax_k(mask[n,16k+4i+j,y,x]) * 4*flow[n,c,y+k/3-1,x+k%3-1]   (ppmstereo.py:185-197)
__global__ __launch_bounds__(256) void convex_upsample_kernel(const float* __restrict__ flow, const float* __restrict__ mask, int mask_ld,
                                                              float* __restrict__ out, int H, int W, int64_t P) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= P * 16) return;
    const int sub = (int)(idx & 15);
    const int64_t pix = idx >> 4;
    const int x = (int)(pix % W), y = (int)((pix / W) % H);
    const int64_t frame = pix / ((int64_t)H * W);
    const float* m = mask + pix * mask_ld + sub;
    float mv[9], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        mv[k] = m[16 * k];
        mx = fmaxf(mx, mv[k]);
    }
    float den = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        mv[k] = expf(mv[k] - mx);
        den += mv[k];
    }
    float o0 = 0.0f, o1 = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
        if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
            const int64_t q = pix + (int64_t)(k / 3 - 1) * W + (k % 3 - 1);
            const float wgt = mv[k] / den;
            o0 += wgt * (4.0f * flow[q * 2]);
            o1 += wgt * (4.0f * flow[q * 2 + 1]);
        }
    }
    const int i = sub >> 2, j = sub & 3;
    const int64_t OW = 4 * (int64_t)W, OHW = 16 * (int64_t)H * W;
    const int64_t o = (frame * 2) * OHW + (int64_t)(4 * y + i) * OW + 4 * x + j;
    out[o] = o0;
    out[o + OHW] = o1;
}
extern "C" int ppms_convex_upsample(const float* flow_nhwc, const float* mask, int mask_ld, float* out, int BT, int H, int W, void* stream) {
    PPMS_REQUIRE(flow_nhwc && mask && out && mask_ld >= 144, "convex_upsample: bad arguments");
    const int64_t P = (int64_t)BT * H * W;
    hipLaunchKernelGGL(convex_upsample_kernel, dim3(ceil_div(P * 16, 256)), dim3(256), 0, (hipStream_t)stream, flow_nhwc, mask, mask_ld,
                       out, H, W, P);
    return ppms_check_launch("convex_upsample");
}

// PPMStereo.convex_upsample_3d, ppmstereo.py:199-228 (use_convex_3d=True): 27 neighbours (kt, ky, kx) of the (t, y, x) volume,
// out[t][c][4y+i][4x+j] = sum_k softmax_k(mask[t][16k + 4i + j][y][x]) * 4 flow[t+kt-1][c][y+ky-1][x+kx-1], zero padded
// (unfoldNd.UnfoldNd([3,3,3], padding=1): k = (kt*3 + ky)*3 + kx).  One thread = one (pixel, sub-position i*4+j).
__global__ __launch_bounds__(256) void convex_upsample3d_kernel(const float* __restrict__ flow, const float* __restrict__ mask, int mask_ld,
                                                                float* __restrict__ out, int T, int H, int W, int t_halo, int64_t P) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= P * 16) return;
    const int sub = (int)(idx & 15);
    const int64_t pix = idx >> 4;
    const int x = (int)(pix % W), y = (int)((pix / W) % H);
    const int64_t frame = pix / ((int64_t)W * H);
    const float* mp = mask + pix * mask_ld + sub;
    float mv[27];
    float mx = mp[0];
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        mv[k] = mp[16 * k];
        mx = fmaxf(mx, mv[k]);
    }
    float den = 0.0f;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        mv[k] = expf(mv[k] - mx);
        den += mv[k];
    }
    float o0 = 0.0f, o1 = 0.0f;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        const int dt = k / 9 - 1, dy = (k / 3) % 3 - 1, dx = k % 3 - 1;
        const int tt = (int)frame + dt, yy = y + dy, xx = x + dx;
        if ((unsigned)(tt + t_halo) < (unsigned)(T + 2 * t_halo) && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
            const int64_t q = pix + ((int64_t)dt * H + dy) * W + dx;
            const float wgt = mv[k] / den;
            o0 += wgt * (4.0f * flow[q * 2]);
            o1 += wgt * (4.0f * flow[q * 2 + 1]);
        }
    }
    const int i = sub >> 2, j = sub & 3;
    const int64_t OW = 4 * (int64_t)W, OHW = 16 * (int64_t)H * W;
    const int64_t o = (frame * 2) * OHW + (int64_t)(4 * y + i) * OW + 4 * x + j;
    out[o] = o0;
    out[o + OHW] = o1;
}
extern "C" int ppms_convex_upsample_3d(const float* flow_nhwc, const float* mask, int mask_ld, float* out, int T, int H, int W, int t_halo, void* stream) {
    PPMS_REQUIRE(flow_nhwc && mask && out && mask_ld >= 432 && T > 0 && H > 0 && W > 0 && t_halo >= 0, "convex_upsample_3d: bad arguments");
    const int64_t P = (int64_t)T * H * W;
    hipLaunchKernelGGL(convex_upsample3d_kernel, dim3(ceil_div(P * 16, 256)), dim3(256), 0, (hipStream_t)stream, flow_nhwc, mask, mask_ld,
                       out, T, H, W, t_halo, P);
    return ppms_check_launch("convex_upsample_3d");
}
