// Glue around the loop: the NCHW / NHWC / SP / fp32 layout converters, the bilinear resize, the SP resize-and-blend between scales and the
// pre-loop pool / axpby / context mix.  Called from ppmstereo_amd/engine.py, ppmstereo.py, encoder.py, cnet.py, update.py and sst.py.
#include "common.h"

// ------------------------------------------------------------------------------------------------ layout converters
// tiled transposes between [frame][C][HW] (NCHW) and [frame*HW][ld] (channel-last); 32x32 tiles through LDS
enum { CV_F32 = 0, CV_SP = 1 };
template <int DST_KIND>
__global__ __launch_bounds__(256) void nchw_to_cl_kernel(const float* __restrict__ src, float* __restrict__ dst_f32, int dst_ld,
                                                         ppms_sp dst_sp, int C, int HW) {
    __shared__ float tile[32][33];
    const int frame = blockIdx.z;
    const int c0 = blockIdx.y * 32, p0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 8 rows per pass
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, p = p0 + tx;
        tile[i][tx] = (c < C && p < HW) ? src[((int64_t)frame * C + c) * HW + p] : 0.0f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int p = p0 + i, c = c0 + tx;
        if (p < HW && c < C) {
            const float v = tile[tx][i];
            const int64_t pix = (int64_t)frame * HW + p;
            if (DST_KIND == CV_F32) {
                dst_f32[pix * dst_ld + c] = v;
            } else {
                bf16_t hi, lo;
                split_bf16(v, hi, lo);
                ((bf16_t*)dst_sp.hi)[pix * dst_sp.ld + c] = hi;
                ((bf16_t*)dst_sp.lo)[pix * dst_sp.ld + c] = lo;
            }
        }
    }
}
template <int SRC_KIND>
__global__ __launch_bounds__(256) void cl_to_nchw_kernel(const float* __restrict__ src_f32, int src_ld, ppms_sp src_sp,
                                                         float* __restrict__ dst, int C, int HW) {
    __shared__ float tile[32][33];
    const int frame = blockIdx.z;
    const int c0 = blockIdx.y * 32, p0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int p = p0 + i, c = c0 + tx;
        float v = 0.0f;
        if (p < HW && c < C) {
            const int64_t pix = (int64_t)frame * HW + p;
            if (SRC_KIND == CV_F32)
                v = src_f32[pix * src_ld + c];
            else
                v = join_bf16(((const bf16_t*)src_sp.hi)[pix * src_sp.ld + c], ((const bf16_t*)src_sp.lo)[pix * src_sp.ld + c]);
        }
        tile[i][tx] = v;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, p = p0 + tx;
        if (c < C && p < HW) dst[((int64_t)frame * C + c) * HW + p] = tile[tx][i];
    }
}

extern "C" int ppms_nchw_to_sp(const float* src, ppms_sp dst, int BT, int C, int HW, void* stream) {
    PPMS_REQUIRE(src && dst.hi && dst.lo && dst.ld >= C, "nchw_to_sp: bad arguments");
    hipLaunchKernelGGL(nchw_to_cl_kernel<CV_SP>, dim3(ceil_div(HW, 32), ceil_div(C, 32), BT), dim3(256), 0, (hipStream_t)stream, src,
                       (float*)nullptr, 0, dst, C, HW);
    return ppms_check_launch("nchw_to_sp");
}
extern "C" int ppms_nchw_to_nhwc(const float* src, float* dst, int dst_ld, int BT, int C, int HW, void* stream) {
    PPMS_REQUIRE(src && dst && dst_ld >= C, "nchw_to_nhwc: bad arguments");
    ppms_sp none = {nullptr, nullptr, 0, 0};
    hipLaunchKernelGGL(nchw_to_cl_kernel<CV_F32>, dim3(ceil_div(HW, 32), ceil_div(C, 32), BT), dim3(256), 0, (hipStream_t)stream, src, dst,
                       dst_ld, none, C, HW);
    return ppms_check_launch("nchw_to_nhwc");
}
extern "C" int ppms_sp_to_nchw(ppms_sp src, float* dst, int BT, int C, int HW, void* stream) {
    PPMS_REQUIRE(dst && src.hi && src.lo && src.ld >= C, "sp_to_nchw: bad arguments");
    hipLaunchKernelGGL(cl_to_nchw_kernel<CV_SP>, dim3(ceil_div(HW, 32), ceil_div(C, 32), BT), dim3(256), 0, (hipStream_t)stream,
                       (const float*)nullptr, 0, src, dst, C, HW);
    return ppms_check_launch("sp_to_nchw");
}
extern "C" int ppms_nhwc_to_nchw(const float* src, int src_ld, float* dst, int BT, int C, int HW, void* stream) {
    PPMS_REQUIRE(src && dst && src_ld >= C, "nhwc_to_nchw: bad arguments");
    ppms_sp none = {nullptr, nullptr, 0, 0};
    hipLaunchKernelGGL(cl_to_nchw_kernel<CV_F32>, dim3(ceil_div(HW, 32), ceil_div(C, 32), BT), dim3(256), 0, (hipStream_t)stream, src,
                       src_ld, none, dst, C, HW);
    return ppms_check_launch("nhwc_to_nchw");
}

__global__ __launch_bounds__(256) void f32_to_sp_kernel(const float* __restrict__ src, int src_ld, ppms_sp dst, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int c = (int)(idx % dst.c);
    const int64_t pix = idx / dst.c;
    bf16_t hi, lo;
    split_bf16(src[pix * src_ld + c], hi, lo);
    ((bf16_t*)dst.hi)[pix * dst.ld + c] = hi;
    ((bf16_t*)dst.lo)[pix * dst.ld + c] = lo;
}
__global__ __launch_bounds__(256) void sp_to_f32_kernel(ppms_sp src, float* __restrict__ dst, int dst_ld, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int c = (int)(idx % src.c);
    const int64_t pix = idx / src.c;
    dst[pix * dst_ld + c] = join_bf16(((const bf16_t*)src.hi)[pix * src.ld + c], ((const bf16_t*)src.lo)[pix * src.ld + c]);
}
extern "C" int ppms_f32_to_sp(const float* src, int src_ld, ppms_sp dst, int64_t pixels, void* stream) {
    PPMS_REQUIRE(src && dst.hi && dst.lo && dst.c > 0, "f32_to_sp: bad arguments");
    const int64_t n = pixels * dst.c;
    hipLaunchKernelGGL(f32_to_sp_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, src, src_ld, dst, n);
    return ppms_check_launch("f32_to_sp");
}
extern "C" int ppms_sp_to_f32(ppms_sp src, float* dst, int dst_ld, int64_t pixels, void* stream) {
    PPMS_REQUIRE(dst && src.hi && src.lo && src.c > 0, "sp_to_f32: bad arguments");
    const int64_t n = pixels * src.c;
    hipLaunchKernelGGL(sp_to_f32_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, dst_ld, n);
    return ppms_check_launch("sp_to_f32");
}

// ------------------------------------------------------------------------------------------------ bilinear resize
// torch upsample_bilinear2d semantics (aten/native/UpSample.h area_pixel_compute_source_index)
__global__ __launch_bounds__(256) void bilinear_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W, int OH, int OW,
                                                       int align, float sh, float sw, float mul, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int ox = (int)(idx % OW);
    const int oy = (int)((idx / OW) % OH);
    const int64_t plane = idx / ((int64_t)OW * OH);
    float fy = align ? sh * oy : fmaxf(sh * (oy + 0.5f) - 0.5f, 0.0f);
    float fx = align ? sw * ox : fmaxf(sw * (ox + 0.5f) - 0.5f, 0.0f);
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + ((y0 < H - 1) ? 1 : 0), x1 = x0 + ((x0 < W - 1) ? 1 : 0);
    const float ly = fy - y0, lx = fx - x0;
    const float hy = 1.0f - ly, hx = 1.0f - lx;
    const float* s = src + plane * H * W;
    const float v = hy * (hx * s[y0 * W + x0] + lx * s[y0 * W + x1]) + ly * (hx * s[y1 * W + x0] + lx * s[y1 * W + x1]);
    dst[idx] = mul * v;
}
extern "C" int ppms_bilinear(const float* src, float* dst, int N, int C, int H, int W, int OH, int OW, int align_corners, float mul,
                             void* stream) {
    PPMS_REQUIRE(src && dst && N > 0 && C > 0 && H > 0 && W > 0 && OH > 0 && OW > 0, "bilinear: bad arguments");
    float sh, sw;
    if (align_corners) {
        sh = OH > 1 ? (float)(H - 1) / (float)(OH - 1) : 0.0f;
        sw = OW > 1 ? (float)(W - 1) / (float)(OW - 1) : 0.0f;
    } else {
        sh = (float)H / (float)OH;
        sw = (float)W / (float)OW;
    }
    const int64_t n = (int64_t)N * C * OH * OW;
    hipLaunchKernelGGL(bilinear_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, H, W, OH, OW, align_corners,
                       sh, sw, mul, n);
    return ppms_check_launch("bilinear");
}

// Scale-to-scale hand-over of the cascade on SP (channel-last split-bf16) tensors, no NCHW round trip:
// dst = a * dst + b * interp(src) with F.interpolate(mode="bilinear", align_corners=True) semantics per frame
// (ppmstereo.py:726-732,763-767: hidden state x2, net = (net_s + interp(net_2s)) / 2).  One thread = one output pixel x 8 channels.
__global__ __launch_bounds__(256) void sp_resize_blend_kernel(ppms_sp src, ppms_sp dst, int H, int W, int OH, int OW, int C8, float sh, float sw,
                                                              float a, float b, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int c = (int)(idx % C8) * 8;
    const int64_t opix = idx / C8;
    const int ox = (int)(opix % OW);
    const int oy = (int)((opix / OW) % OH);
    const int64_t frame = opix / ((int64_t)OW * OH);
    const float fy = sh * oy, fx = sw * ox;
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + ((y0 < H - 1) ? 1 : 0), x1 = x0 + ((x0 < W - 1) ? 1 : 0);
    const float ly = fy - y0, lx = fx - x0;
    const float hy = 1.0f - ly, hx = 1.0f - lx;
    const int64_t base = frame * H * W;
    auto ld8 = [&](int y, int x, float* v) {
        const int64_t o = (base + (int64_t)y * W + x) * src.ld + c;
        const bf16x8 h8 = *(const bf16x8*)((const bf16_t*)src.hi + o), l8 = *(const bf16x8*)((const bf16_t*)src.lo + o);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = join_bf16(h8[j], l8[j]);
    };
    float v00[8], v01[8], v10[8], v11[8];
    ld8(y0, x0, v00);
    ld8(y0, x1, v01);
    ld8(y1, x0, v10);
    ld8(y1, x1, v11);
    const int64_t od = opix * dst.ld + c;
    float d[8];
    if (a != 0.0f) {
        const bf16x8 h8 = *(const bf16x8*)((const bf16_t*)dst.hi + od), l8 = *(const bf16x8*)((const bf16_t*)dst.lo + od);
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] = join_bf16(h8[j], l8[j]);
    }
    bf16x8 oh, ol;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float v = hy * (hx * v00[j] + lx * v01[j]) + ly * (hx * v10[j] + lx * v11[j]);
        const float y = (a != 0.0f) ? a * d[j] + b * v : b * v;
        bf16_t hh, ll;
        split_bf16(y, hh, ll);
        oh[j] = hh;
        ol[j] = ll;
    }
    *(bf16x8*)((bf16_t*)dst.hi + od) = oh;
    *(bf16x8*)((bf16_t*)dst.lo + od) = ol;
}
extern "C" int ppms_sp_resize_blend(ppms_sp src, ppms_sp dst, int N, int H, int W, int OH, int OW, float a, float b, void* stream) {
    PPMS_REQUIRE(src.hi && src.lo && dst.hi && dst.lo && N > 0 && H > 0 && W > 0 && OH > 0 && OW > 0, "sp_resize_blend: bad arguments");
    PPMS_REQUIRE(src.c == dst.c && src.c % 8 == 0 && src.ld % 8 == 0 && dst.ld % 8 == 0, "sp_resize_blend: channel views must match, multiples of 8");
    PPMS_REQUIRE((((uintptr_t)src.hi | (uintptr_t)src.lo | (uintptr_t)dst.hi | (uintptr_t)dst.lo) & 15) == 0, "sp_resize_blend: views must be 16-B aligned");
    const float sh = OH > 1 ? (float)(H - 1) / (float)(OH - 1) : 0.0f, sw = OW > 1 ? (float)(W - 1) / (float)(OW - 1) : 0.0f;
    const int64_t n = (int64_t)N * OH * OW * (src.c / 8);
    hipLaunchKernelGGL(sp_resize_blend_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, H, W, OH, OW, src.c / 8, sh, sw, a, b, n);
    return ppms_check_launch("sp_resize_blend");
}

// ------------------------------------------------------------------------------------------------ pre-loop glue of PPMStereo.forward
// (ppmstereo.py:620-682, between the encoders and the loop: the caller of the hot path)
// F.avg_pool2d(x, k, stride=k) on NCHW fp32 planes (k = 4: 1/4 -> 1/16 features :649-650, k = 2: :666-671)
__global__ __launch_bounds__(256) void avgpool_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W, int k, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int OW = W / k, OH = H / k;
    const int ox = (int)(idx % OW), oy = (int)((idx / OW) % OH);
    const int64_t plane = idx / ((int64_t)OW * OH);
    const float* s = src + plane * H * W + (int64_t)oy * k * W + ox * k;
    float acc = 0.0f;
    for (int dy = 0; dy < k; ++dy)
        for (int dx = 0; dx < k; ++dx) acc += s[dy * W + dx];
    dst[idx] = acc / (float)(k * k);
}
extern "C" int ppms_avgpool(const float* src, float* dst, int planes, int H, int W, int k, void* stream) {
    PPMS_REQUIRE(src && dst && planes > 0 && k > 0 && H >= k && W >= k, "avgpool: bad arguments");
    const int64_t n = (int64_t)planes * (H / k) * (W / k);
    hipLaunchKernelGGL(avgpool_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, H, W, k, n);
    return ppms_check_launch("avgpool");
}
// out = a * x + b * y[i mod period]  (period = n: plain axpby; period = C*H*W: y broadcast over frames, the positional encoding
// of :327-333; a = b = 0.5: the feature / context averages of :627-628, :666-671)
__global__ __launch_bounds__(256) void axpby_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ out, float a, float b,
                                                    int64_t period, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < n) out[idx] = a * x[idx] + b * y[idx % period];
}
extern "C" int ppms_axpby(const float* x, const float* y, float* out, float a, float b, int64_t period, int64_t n, void* stream) {
    PPMS_REQUIRE(x && y && out && n > 0 && period > 0, "axpby: bad arguments");
    hipLaunchKernelGGL(axpby_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, x, y, out, a, b, period, n);
    return ppms_check_launch("axpby");
}
// net = tanh((f[:, :128] + c[:, :128]) / 2), inp = relu((f[:, 128:] + c[:, 128:]) / 2)   (:620-632, :660-664, :673-682);
// f, c: NCHW (N, 256, HW); net, inp: NCHW (N, 128, HW).  tanhf: the library-accurate form (one-off per scale).
__global__ __launch_bounds__(256) void ctx_mix_kernel(const float* __restrict__ f, const float* __restrict__ c, float* __restrict__ net,
                                                      float* __restrict__ inp, int64_t chw, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;      // over N * 128 * HW
    if (idx >= n) return;
    const int64_t frame = idx / chw, rem = idx - frame * chw;
    const int64_t src = frame * 2 * chw + rem;
    net[idx] = tanhf((f[src] + c[src]) / 2.0f);
    const float v = (f[src + chw] + c[src + chw]) / 2.0f;
    inp[idx] = v < 0.0f ? 0.0f : v;
}
extern "C" int ppms_ctx_mix(const float* fmap, const float* ctx, float* net, float* inp, int N, int HW, void* stream) {
    PPMS_REQUIRE(fmap && ctx && net && inp && N > 0 && HW > 0, "ctx_mix: bad arguments");
    const int64_t chw = (int64_t)128 * HW, n = (int64_t)N * chw;
    hipLaunchKernelGGL(ctx_mix_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, fmap, ctx, net, inp, chw, n);
    return ppms_check_launch("ctx_mix");
}
