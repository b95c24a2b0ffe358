// Pieces of the feature encoder `BasicEncoder(output_dim=256, norm_fn="instance")` (fnet, SURVEY.md section 8 row f3;
// /root/reference/models/core/extractor.py:302-423) that are not convolutions.  The convolutions run on the implicit-GEMM
// kernels of conv_gemm2/5.hip; the two stride-2 layers (conv1 7x7 s2, layer2.0 conv1 3x3 s2 + its 1x1 s2 skip) become stride-1
// convolutions on a 2x2 space-to-depth copy of their input (host side: ppmstereo_amd/encoder.py re-lays the weights).
#include "common.h"

namespace {

// ---- space to depth, factor k: dst[(n, i, j)][phase * C + c] = src[(n, k i + dy, k j + dx)][c], phase = k dy + dx -------------
// image form: src is the NCHW fp32 image batch the reference hands to its encoders (3 channels); channels >= k*k*C of dst are zeroed
__global__ __launch_bounds__(256) void img_s2d_kernel(const float* __restrict__ img, ppms_sp dst, int C, int H, int W, int k, int64_t npix) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;          // one thread = one output pixel x 8 channels
    const int groups = dst.c >> 3;
    if (idx >= npix * groups) return;
    const int g8 = (int)(idx % groups);
    const int64_t p = idx / groups;
    const int OW = W / k, OH = H / k;
    const int j = (int)(p % OW), i = (int)((p / OW) % OH);
    const int64_t n = p / ((int64_t)OW * OH);
    bf16x8 oh, ol;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int ch = g8 * 8 + e;
        float v = 0.0f;
        if (ch < k * k * C) {
            const int ph = ch / C, c = ch - ph * C;
            v = img[((n * C + c) * H + k * i + ph / k) * W + k * j + ph % k];
        }
        bf16_t hh, ll;
        split_bf16(v, hh, ll);
        oh[e] = hh;
        ol[e] = ll;
    }
    const int64_t od = p * dst.ld + g8 * 8;
    *(bf16x8*)((bf16_t*)dst.hi + od) = oh;
    *(bf16x8*)((bf16_t*)dst.lo + od) = ol;
}

// decoded video -> the first-layer operands of both encoders in one launch (ppms_video_ingest_u8 / ppms_video_ingest_yuv420 / ppms_video_ingest_yuv / ppms_video_ingest_raw):
// what normalisation (a table the caller built with the float path's own torch expression: 256 entries, or 1 << depth for a source whose
// table_by_depth is true, which also answers levels()), replicate padding (clamped source
// coordinate), torch.cat([left, right]) and the two img_s2d launches produce from the fp32 images.  Thread = one output pixel x 8 channels
// of one destination, as in img_s2d_kernel: indices [0, nf) serve the k = 2 operand of the 2 N images (left frames, then right frames),
// [nf, total) the k = 4 operand of the N left frames.  Where a byte comes from is the Source: source(m, c, y, x) = channel c (R, G, B) of
// pixel (y, x), already clamped into the frame, of image m.  Source rows have arbitrary widths and pitches: byte loads only.
struct rgb_planes_source {                                                // planar RGB bytes, dense rows (ppms_video_ingest_u8)
    const uint8_t *left, *right;
    int64_t frame_stride;
    int N, H0, W0;
    static constexpr bool table_by_depth = false;                         // RGB bytes: the kernel's static 256-entry table
    __device__ int operator()(int64_t m, int c, int y, int x) const {
        const uint8_t* src = m < N ? left + m * frame_stride : right + (m - N) * frame_stride;
        return src[((int64_t)c * H0 + y) * W0 + x];
    }
};

struct yuv420_source {                                                    // pitched Y plane + half-resolution chroma (ppms_video_ingest_yuv420)
    ppms_yuv_view left, right;
    ppms_yuv_matrix mat;
    int N;
    static constexpr bool table_by_depth = false;
    __device__ int operator()(int64_t m, int c, int y, int x) const {
        const bool r = m >= N;
        const int64_t n = r ? m - N : m;
        const uint8_t *py = r ? right.y : left.y, *pu = r ? right.u : left.u, *pv = r ? right.v : left.v;
        const int64_t oy = n * (r ? right.frame_stride_y : left.frame_stride_y) + (int64_t)y * (r ? right.pitch_y : left.pitch_y) + x;
        const int64_t oc = n * (r ? right.frame_stride_c : left.frame_stride_c) + (int64_t)(y >> 1) * (r ? right.pitch_c : left.pitch_c) +
                           (int64_t)(x >> 1) * (r ? right.step_c : left.step_c);      // nearest chroma sample of the clamped luma pixel
        // the three channels of a pixel repeat these loads; they are the same addresses, and the compiler merges them
        const int d = py[oy] - mat.y_off, e = pu[oc] - 128, f = pv[oc] - 128;
        const int acc = mat.cy * d + (c == 0 ? mat.crv * f : c == 1 ? -mat.cgu * e - mat.cgv * f : mat.cbu * e) + (1 << (mat.shift - 1));
        const int q = acc >> mat.shift;                                   // arithmetic shift: floor
        return q < 0 ? 0 : (q > 255 ? 255 : q);
    }
};

// samples of T (bytes, or little-endian 16-bit words holding 10 or 12 bits) with any of the three chroma subsamplings (ppms_video_ingest_yuv):
// yuv420_source's conversion on `depth`-bit samples, RGB levels in [0, 2^depth - 1].  Every stride of the views is in bytes, every offset 64-bit;
// loads are of one T (rows have arbitrary pitches; the host checks that they are even for 16-bit samples).  A sample is masked to `depth` bits
// and the result clamped, so the level is always an index inside the table of 1 << depth entries.
template <class T>
struct yuv_source {
    ppms_yuv_view left, right;
    ppms_yuv_matrix mat;
    int N, depth, lsb, sub_x, sub_y;                                      // uniform: the ppms_yuv_format
    static constexpr bool table_by_depth = true;
    __host__ __device__ int levels() const { return 1 << depth; }
    __device__ int sample(const uint8_t* p, int64_t o) const { return ((int)*(const T*)(p + o) >> lsb) & ((1 << depth) - 1); }
    __device__ int operator()(int64_t m, int c, int y, int x) const {
        const bool r = m >= N;
        const int64_t n = r ? m - N : m;
        const uint8_t *py = r ? right.y : left.y, *pu = r ? right.u : left.u, *pv = r ? right.v : left.v;
        const int64_t oy = n * (r ? right.frame_stride_y : left.frame_stride_y) + (int64_t)y * (r ? right.pitch_y : left.pitch_y) + (int64_t)x * (int)sizeof(T);
        const int64_t oc = n * (r ? right.frame_stride_c : left.frame_stride_c) + (int64_t)(y >> sub_y) * (r ? right.pitch_c : left.pitch_c) +
                           (int64_t)(x >> sub_x) * (r ? right.step_c : left.step_c);  // nearest chroma sample of the clamped luma pixel
        // the three channels of a pixel repeat these loads; they are the same addresses, and the compiler merges them
        const int mid = 1 << (depth - 1), top = (1 << depth) - 1;
        const int d = sample(py, oy) - mat.y_off, e = sample(pu, oc) - mid, f = sample(pv, oc) - mid;
        const int acc = mat.cy * d + (c == 0 ? mat.crv * f : c == 1 ? -mat.cgu * e - mat.cgv * f : mat.cbu * e) + (1 << (mat.shift - 1));
        const int q = acc >> mat.shift;                                   // arithmetic shift: floor
        return q < 0 ? 0 : (q > top ? top : q);
    }
};

// a sensor's raw frames (ppms_video_ingest_raw): one pitched plane of T samples under a 2 x 2 colour-filter mosaic, or monochrome.  The missing
// colours of a pixel are bilinear means of its neighbours (the arithmetic: include/ppms.h); a neighbour outside the frame is REFLECTED without
// repeating the edge (-1 -> 1, n -> n - 2), which keeps its colour.  `pattern` is uniform, and which colour a site carries is parity arithmetic:
// a site is green where (x ^ y ^ (pattern >> 1)) is odd, and rows with (y ^ pattern) even hold the red sites.  (y, x) arrives inside the hs x ws
// frame, and with hs, ws >= 2 (the host refuses less for a colour pattern) so does every reflected neighbour: no load leaves the frame.
template <class T>
struct raw_source {
    ppms_raw_view left, right;
    int N, hs, ws;                                                        // frames per view, the SOURCE frame size
    int depth, lsb, pattern, black, gain_r, gain_g, gain_b, shift;        // uniform: the ppms_raw_format
    static constexpr bool table_by_depth = true;
    __host__ __device__ int levels() const { return 1 << depth; }
    __device__ int operator()(int64_t m, int c, int y, int x) const {
        const bool r = m >= N;
        const uint8_t* p = (r ? right.data : left.data) + (r ? m - N : m) * (r ? right.frame_stride : left.frame_stride);
        const int64_t pitch = r ? right.pitch : left.pitch;
        const int top = (1 << depth) - 1;
        // the three channels of a pixel repeat these loads; they are the same addresses, and the compiler merges them
        const auto s = [&](int yy, int xx) { return ((int)*(const T*)(p + yy * pitch + (int64_t)xx * (int)sizeof(T)) >> lsb) & top; };
        int v;
        if (pattern == 4) {                                               // MONO
            v = s(y, x);
        } else {
            const int ym = y > 0 ? y - 1 : 1, yp = y < hs - 1 ? y + 1 : hs - 2, xm = x > 0 ? x - 1 : 1, xp = x < ws - 1 ? x + 1 : ws - 2;
            const bool green = ((x ^ y ^ (pattern >> 1)) & 1) != 0, red_row = ((y ^ pattern) & 1) == 0;
            if (c == (green ? 1 : (red_row ? 0 : 2)))
                v = s(y, x);
            else if (green)                                               // R or B at a green site: the two neighbours that carry it
                v = (c == 0) == red_row ? (s(y, xm) + s(y, xp) + 1) >> 1 : (s(ym, x) + s(yp, x) + 1) >> 1;
            else if (c == 1)                                              // G at a red or blue site
                v = (s(ym, x) + s(yp, x) + s(y, xm) + s(y, xp) + 2) >> 2;
            else                                                          // B at a red site, R at a blue site
                v = (s(ym, xm) + s(ym, xp) + s(yp, xm) + s(yp, xp) + 2) >> 2;
        }
        const int q = ((v - black) * (c == 0 ? gain_r : c == 1 ? gain_g : gain_b) + (1 << (shift - 1))) >> shift;     // arithmetic shift: floor
        return q < 0 ? 0 : (q > top ? top : q);
    }
};

// a source behind a rectification map (ppms_video_ingest_u8_remap / ppms_video_ingest_yuv420_remap; the arithmetic: include/ppms.h): (y, x) is a
// pixel of the RECTIFIED frame, the view's map names its four taps in the inner source's frame of hs x ws, and the blend is integer.  Every
// tap coordinate is clamped into that frame before the inner source sees it, whatever the map holds: in constant mode a tap outside the frame
// contributes `fill` instead of what lies at the clamped address.
template <class Inner>
struct remapped_source {
    Inner inner;                                                          // built with the source frame size
    ppms_remap_view left, right;
    int N;
    static constexpr bool table_by_depth = Inner::table_by_depth;
    __host__ __device__ int levels() const { return inner.levels(); }      // (asked of a table_by_depth source only)
    __device__ int operator()(int64_t m, int c, int y, int x) const {
        const bool r = m >= N;
        const int64_t o = (int64_t)y * (r ? right.pitch : left.pitch) + x;
        // the three channels of a pixel repeat these loads; they are the same addresses, and the compiler merges them
        const short2 xy = ((const short2*)(r ? right.xy : left.xy))[o];
        const int fr = (r ? right.frac : left.frac)[o];
        const int fx = fr & 31, fy = (fr >> 5) & 31;
        const int hs = left.hs, ws = left.ws, border = r ? right.border : left.border, fill = r ? right.fill : left.fill;
        int acc = 512;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int yy = (int)xy.y + (t >> 1), xx = (int)xy.x + (t & 1);    // int16 + 1: 32-bit arithmetic
            const bool outside = yy < 0 || yy > hs - 1 || xx < 0 || xx > ws - 1;
            const int cy = yy < 0 ? 0 : (yy > hs - 1 ? hs - 1 : yy), cx = xx < 0 ? 0 : (xx > ws - 1 ? ws - 1 : xx);
            const int p = border && outside ? fill : inner(m, c, cy, cx);
            acc += ((t & 1) ? fx : 32 - fx) * ((t >> 1) ? fy : 32 - fy) * p;
        }
        return acc >> 10;                                                 // weights sum to 1024: in [0, the inner source's top level]
    }
};

template <class Source>
__global__ __launch_bounds__(256) void video_ingest_kernel(Source source, int N, int H0, int W0, int pad_left, int pad_top, int H, int W,
                                                           const float* __restrict__ lut, ppms_sp dst_fnet, ppms_sp dst_cnet, int64_t nf, int64_t total) {
    const float* tab;
    if constexpr (Source::table_by_depth) {                               // 1 << depth entries of dynamic LDS (sized by the launch): every thread fills
        extern __shared__ float level_tab[];                              // its stride of the table, and leaves only behind the barrier
        for (int i = threadIdx.x, n = source.levels(); i < n; i += 256) level_tab[i] = lut[i];
        tab = level_tab;
    } else {
        __shared__ float byte_tab[256];
        byte_tab[threadIdx.x] = lut[threadIdx.x];
        tab = byte_tab;
    }
    __syncthreads();
    int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const bool fnet = idx < nf;
    if (!fnet) idx -= nf;
    const ppms_sp dst = fnet ? dst_fnet : dst_cnet;
    const int ks = fnet ? 1 : 2, k = 1 << ks;                             // k = 2 (fnet) or 4 (cnet stem)
    const int groups = dst.c >> 3;
    const int g8 = (int)(idx % groups);
    const int64_t p = idx / groups;
    const int OW = W >> ks, OH = H >> ks;
    const int j = (int)(p % OW), i = (int)((p / OW) % OH);
    const int64_t m = p / ((int64_t)OW * OH);                             // image: left frames 0 .. N - 1, then the right frames
    bf16x8 oh, ol;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int ch = g8 * 8 + e;
        float v = 0.0f;
        if (ch < k * k * 3) {
            const int ph = ch / 3, c = ch - ph * 3;
            int y = k * i + (ph >> ks) - pad_top, x = k * j + (ph & (k - 1)) - pad_left;
            y = y < 0 ? 0 : (y > H0 - 1 ? H0 - 1 : y);                    // replicate padding
            x = x < 0 ? 0 : (x > W0 - 1 ? W0 - 1 : x);
            v = tab[source(m, c, y, x)];
        }
        bf16_t hh, ll;
        split_bf16(v, hh, ll);
        oh[e] = hh;
        ol[e] = ll;
    }
    const int64_t od = p * dst.ld + g8 * 8;
    *(bf16x8*)((bf16_t*)dst.hi + od) = oh;
    *(bf16x8*)((bf16_t*)dst.lo + od) = ol;
}

// split-plane form: pure copies of 16-B channel groups (both planes)
__global__ __launch_bounds__(256) void sp_s2d_kernel(ppms_sp src, ppms_sp dst, int H, int W, int64_t npix) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;          // one thread = one output pixel x 8 channels
    const int C = src.c, groups = (4 * C) >> 3;
    if (idx >= npix * groups) return;
    const int g8 = (int)(idx % groups);
    const int64_t p = idx / groups;
    const int OW = W >> 1, OH = H >> 1;
    const int j = (int)(p % OW), i = (int)((p / OW) % OH);
    const int64_t n = p / ((int64_t)OW * OH);
    const int ch = g8 * 8, ph = ch / C, c = ch - ph * C;                  // C % 8 == 0: a group never straddles two phases
    const int64_t sp = ((n * H + 2 * i + (ph >> 1)) * W + 2 * j + (ph & 1)) * src.ld + c;
    const int64_t od = p * dst.ld + ch;
    *(bf16x8*)((bf16_t*)dst.hi + od) = *(const bf16x8*)((const bf16_t*)src.hi + sp);
    *(bf16x8*)((bf16_t*)dst.lo + od) = *(const bf16x8*)((const bf16_t*)src.lo + sp);
}

// ---- InstanceNorm2d(affine=False, eps): per (sample, channel) mean and biased variance over the H*W pixels -------------------
// x: channel-last fp32 [N*HW][ld] (a conv's fp32 output).  Two launches, deterministic:
//  1. one workgroup = one sample x 32 channels x one of S pixel slices: slice mean m_s as fp32 rounds it, then the slice sums of
//     d = x - m_s and of d^2 (two passes over an L2-resident slice: no cancellation) -> part[n][s][c] = (m_s, M2_s, r_s, -);
//  2. one thread per (sample, channel) merges the S slices in slice order, in float64, about the first slice's mean m_0:
//     with e = m_s - m_0: A += n_s e + r_s, Q += M2_s + 2 e r_s + n_s e^2 (the sums of x - m_0 and of its square over the slice, exactly),
//     mean = m_0 + A / HW, M2 = Q - A^2 / HW -> stats[n][c] = (mean, 1 / sqrt(M2 / HW + eps)).
// r_s is what fp32 drops from the slice mean.  Without it a map whose mean is large against its spread (|mean| = 1000 sigma) lost 1e-5 of
// rstd: the differences between slice means, which carry 1 / n_s of the variance, were taken between values rounded at the mean's magnitude.
static int in_slices_host(int N, int HW, int C) {                      // enough workgroups to fill the chip, >= 64 pixels each
    const int per = (int)ceil_div(C, 32) * N;
    int S = 1024 / (per > 0 ? per : 1);
    const int smax = HW / 64;
    if (S > smax) S = smax;
    return S < 1 ? 1 : S;
}

// thread = 4 channels (one 16-byte load) of every 32nd pixel of the slice: 8 threads cover the workgroup's 32 channels, 32 pixel rows per step
// (the 4-byte-per-lane form of round 2 ran at 2.4 TB/s: 4x the load instructions)
__global__ __launch_bounds__(256) void instnorm_part_kernel(const float* __restrict__ x, int ld, int HW, int C, int S, float* __restrict__ part) {
    __shared__ float red[2][4][32];                                        // [quantity][wave][channel]
    __shared__ float mean_s[32];
    const int n = blockIdx.y, c0 = blockIdx.x * 32, s = blockIdx.z;
    const int q = threadIdx.x & 7, row = threadIdx.x >> 3;                // channels c0 + 4 q .. + 3, pixel rows row, row + 32, ...
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;           // a wave = 8 pixel rows x the 8 channel quads
    const int c = c0 + 4 * q;
    const int chunk = (HW + S - 1) / S;
    const int p0 = s * chunk, p1 = (p0 + chunk < HW) ? p0 + chunk : HW;
    const int cnt = p1 - p0;
    const float* xp = x + (int64_t)n * HW * ld + c;
    const bool vec = (ld & 3) == 0 && c + 4 <= C && (((uintptr_t)x) & 15) == 0;      // (uniform per thread; the tail channels of a C % 4 != 0 layer go one by one)
    auto load4 = [&](int p, float (&v)[4]) {
        if (vec) {
            const f32x4 t = *(const f32x4*)(xp + (int64_t)p * ld);
            v[0] = t[0], v[1] = t[1], v[2] = t[2], v[3] = t[3];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (c + j < C) ? xp[(int64_t)p * ld + j] : 0.0f;
        }
    };
    // sum over the 32 row groups, fixed order: a butterfly over the 8 rows of a wave, then (once the workgroup has synchronised) the 4
    // waves in wave order by sum_waves.  The second pass has two quantities to sum: in this form they share one barrier and one small
    // LDS array (measured: instnorm_stats takes what it took with the serial 32-row LDS sum of one quantity, within 1 us at the product's shapes).
    auto rows_to_lds = [&](float (&acc)[4], int k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float t = acc[j];
            t += __shfl_xor(t, 8);
            t += __shfl_xor(t, 16);
            t += __shfl_xor(t, 32);
            if (lane < 8) red[k][wave][4 * q + j] = t;
        }
    };
    auto sum_waves = [&](int k) { return ((red[k][0][threadIdx.x] + red[k][1][threadIdx.x]) + red[k][2][threadIdx.x]) + red[k][3][threadIdx.x]; };
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int p = p0 + row; p < p1; p += 32) {
        float v[4];
        load4(p, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += v[j];
    }
    rows_to_lds(acc, 0);
    __syncthreads();
    if (threadIdx.x < 32) mean_s[threadIdx.x] = sum_waves(0) * (cnt > 0 ? 1.0f / (float)cnt : 0.0f);
    __syncthreads();
    float mean[4], rem[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 4; ++j) mean[j] = mean_s[4 * q + j], acc[j] = 0.0f;
    for (int p = p0 + row; p < p1; p += 32) {                            // second pass: the slice is L2 resident
        float v[4];
        load4(p, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = v[j] - mean[j];
            acc[j] += d * d;
            rem[j] += d;
        }
    }
    rows_to_lds(acc, 0);
    rows_to_lds(rem, 1);
    __syncthreads();
    if (threadIdx.x < 32 && c0 + (int)threadIdx.x < C) {
        *(f32x4*)(part + (((int64_t)n * S + s) * C + c0 + threadIdx.x) * 4) = (f32x4){mean_s[threadIdx.x], sum_waves(0), sum_waves(1), 0.0f};
    }
}

__global__ __launch_bounds__(256) void instnorm_merge_kernel(const float* __restrict__ part, int HW, int C, int S, float eps, int total, float* __restrict__ stats) {
    const int idx = blockIdx.x * 256 + threadIdx.x;                        // (n, c)
    if (idx >= total) return;
    const int n = idx / C, c = idx - n * C;
    const int chunk = (HW + S - 1) / S;
    const f32x4* pp = (const f32x4*)part + (int64_t)n * S * C + c;                    // slice s at pp[s * C]: (m_s, M2_s, r_s, -)
    const double m0 = (double)pp[0][0];                                               // (slice 0 is never empty)
    double a = 0.0, q = 0.0;
    for (int s0 = 0; s0 < S; s0 += 8) {          // the 8 loads of a group are in flight together (one by one the S ~ 50 dependent-looking
        f32x4 o[8];                              // round trips were the kernel: 13.6 us); the sums stay in slice order
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = pp[(int64_t)(s0 + j < S ? s0 + j : S - 1) * C];      // unconditional (a branch per load serialises them)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int s = s0 + j;
            const int p0 = s * chunk, p1 = (p0 + chunk < HW) ? p0 + chunk : HW;
            const double nb = (double)(p1 - p0);
            if (s >= S || nb <= 0.0) continue;
            const double e = (double)o[j][0] - m0, rs = (double)o[j][2];
            a += nb * e + rs;
            q += (double)o[j][1] + 2.0 * e * rs + nb * e * e;
        }
    }
    const double m2 = q - a * a / (double)HW;
    stats[(int64_t)idx * 2] = (float)(m0 + a / (double)HW);
    stats[(int64_t)idx * 2 + 1] = (float)(1.0 / sqrt((m2 > 0.0 ? m2 : 0.0) / (double)HW + (double)eps));
}

// y = (x - mean) * rstd  [+ res]  [relu]  -> split planes; channels >= C of `out` (padding of the next conv's input) are zeroed
__global__ __launch_bounds__(256) void instnorm_apply_kernel(const float* __restrict__ x, int ld, const float* __restrict__ stats, ppms_sp res, int relu,
                                                             ppms_sp out, int HW, int C, int64_t npix) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;          // one thread = one pixel x 8 channels
    const int groups = out.c >> 3;
    if (idx >= npix * groups) return;
    const int g8 = (int)(idx % groups);
    const int64_t p = idx / groups;
    const int64_t n = p / HW;
    const int c0 = g8 * 8;
    bf16x8 oh, ol, rh, rl;
    const bool has_res = res.hi != nullptr && c0 < C;
    if (has_res) {
        rh = *(const bf16x8*)((const bf16_t*)res.hi + p * res.ld + c0);
        rl = *(const bf16x8*)((const bf16_t*)res.lo + p * res.ld + c0);
    }
    float xv[8], sm[8], sr[8];
    if (c0 + 8 <= C && (ld & 3) == 0 && (C & 1) == 0 && ((((uintptr_t)x) | ((uintptr_t)stats)) & 15) == 0) {       // 16-byte loads: the pixel's 8 values and their 8 (mean, rstd) pairs
        const f32x4 a = *(const f32x4*)(x + p * ld + c0), b = *(const f32x4*)(x + p * ld + c0 + 4);
        const f32x4* st4 = (const f32x4*)(stats + ((int64_t)n * C + c0) * 2);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            xv[e] = a[e], xv[4 + e] = b[e];
            const f32x4 t = st4[e];
            sm[2 * e] = t[0], sr[2 * e] = t[1], sm[2 * e + 1] = t[2], sr[2 * e + 1] = t[3];
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = c0 + e;
            const bool in = c < C;
            xv[e] = in ? x[p * ld + c] : 0.0f;
            sm[e] = in ? stats[((int64_t)n * C + c) * 2] : 0.0f;
            sr[e] = in ? stats[((int64_t)n * C + c) * 2 + 1] : 0.0f;
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = c0 + e;
        float v = 0.0f;
        if (c < C) {
            v = (xv[e] - sm[e]) * sr[e];
            if (has_res) v += join_bf16(rh[e], rl[e]);
            if (relu) v = fmaxf(v, 0.0f);
        }
        bf16_t hh, ll;
        split_bf16(v, hh, ll);
        oh[e] = hh;
        ol[e] = ll;
    }
    const int64_t od = p * out.ld + c0;
    *(bf16x8*)((bf16_t*)out.hi + od) = oh;
    *(bf16x8*)((bf16_t*)out.lo + od) = ol;
}

// ================================================================================================ cnet (ConvNeXt-V2 + FPN) pieces
// (/root/reference/models/core/convnext.py: SURVEY.md section 8 row f5)
// nn.Upsample(scale_factor=2), nearest (:226-238): dst[(n, y, x)] = src[(n, y / 2, x / 2)]; split planes, 16-B channel groups
__global__ __launch_bounds__(256) void sp_upsample2_kernel(ppms_sp src, ppms_sp dst, int H, int W, int64_t npix) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;          // one thread = one OUTPUT pixel x 8 channels
    const int groups = src.c >> 3;
    if (idx >= npix * groups) return;
    const int g8 = (int)(idx % groups);
    const int64_t p = idx / groups;
    const int OW = 2 * W, OH = 2 * H;
    const int x = (int)(p % OW), y = (int)((p / OW) % OH);
    const int64_t n = p / ((int64_t)OW * OH);
    const int64_t sp = ((n * H + (y >> 1)) * W + (x >> 1)) * src.ld + g8 * 8;
    const int64_t od = p * dst.ld + g8 * 8;
    *(bf16x8*)((bf16_t*)dst.hi + od) = *(const bf16x8*)((const bf16_t*)src.hi + sp);
    *(bf16x8*)((bf16_t*)dst.lo + od) = *(const bf16x8*)((const bf16_t*)src.lo + sp);
}

// depthwise 7 x 7 convolution + bias (Block.dwconv, :60): split planes in, fp32 channel-last out.  Same scheme as dwconv_gelu_kernel
// (small_ops.hip): one thread = a run of 4 pixels along x times 8 channels, per kernel row the 4 + 6 window positions are loaded once
// (16-byte loads of both planes) and the 7 taps sweep them from registers; a workgroup serves one block of <= 64 channels (blockIdx.y)
// whose weights sit in LDS transposed to [tap][channel].  Weights [C][49] as in the state_dict.
constexpr int DWP_PX = 4;
__global__ __launch_bounds__(256) void dwconv_plain_kernel(ppms_sp x, float* __restrict__ y, int ldy, const float* __restrict__ w, const float* __restrict__ b,
                                                           int H, int W, int64_t rows) {
    constexpr int K = 7, R = 3, NW = DWP_PX + K - 1;
    __shared__ __attribute__((aligned(16))) float wl[K * K * 64];
    const int cb = blockIdx.y * 64;                                        // first channel of this workgroup's block
    const int cn = (x.c - cb) < 64 ? (x.c - cb) : 64;                      // channels in it (multiple of 8)
    for (int i = threadIdx.x; i < K * K * cn; i += 256) {
        const int c = i % cn, tap = i / cn;
        wl[tap * 64 + c] = w[(cb + c) * K * K + tap];
    }
    __syncthreads();
    const int groups = cn >> 3;
    const int rpr = (W + DWP_PX - 1) / DWP_PX;                             // runs per image row
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * rpr * groups) return;
    const int cl = (int)(idx % groups) * 8, c0 = cb + cl;
    const int64_t run = idx / groups;
    const int px0 = (int)(run % rpr) * DWP_PX;
    const int64_t row = run / rpr;                                         // sample * H + y
    const int py = (int)(row % H);
    const int64_t pix0 = row * W + px0;
    const bf16_t* xh = (const bf16_t*)x.hi + c0;
    const bf16_t* xl = (const bf16_t*)x.lo + c0;
    float acc[DWP_PX][8];
    {
        const f32x4 b0 = *(const f32x4*)(b + c0), b1 = *(const f32x4*)(b + c0 + 4);
#pragma unroll
        for (int p = 0; p < DWP_PX; ++p)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[p][j] = j < 4 ? b0[j & 3] : b1[j & 3];
    }
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
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            const f32x4 w0 = *(const f32x4*)(wl + (ky * K + kx) * 64 + cl), w1 = *(const f32x4*)(wl + (ky * K + kx) * 64 + cl + 4);
#pragma unroll
            for (int p = 0; p < DWP_PX; ++p)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[p][j] += win[p + kx][j] * (j < 4 ? w0[j & 3] : w1[j & 3]);
        }
    }
#pragma unroll
    for (int p = 0; p < DWP_PX; ++p) {
        if (px0 + p >= W) break;
        float* o = y + (pix0 + p) * ldy + c0;
        *(f32x4*)o = (f32x4){acc[p][0], acc[p][1], acc[p][2], acc[p][3]};
        *(f32x4*)(o + 4) = (f32x4){acc[p][4], acc[p][5], acc[p][6], acc[p][7]};
    }
}

// LayerNorm over the channels of a pixel, any C (convnext.py:11-35, eps 1e-6: both data formats are this per-pixel op on
// channel-last data): x fp32 [pixel][ld] -> split planes.  One wave per pixel, lanes stride the channels.
__global__ __launch_bounds__(256) void layernorm_any_kernel(const float* __restrict__ x, int ld, const float* __restrict__ w, const float* __restrict__ b,
                                                            float eps, ppms_sp out, int64_t pixels, int C) {
    // a wave per pixel; a lane owns 8 consecutive channels per round of 512 (two 16-byte loads, one 16-byte store per plane); the pixel's
    // values stay in registers between the three passes (C <= 1024: the host checks); sums in lane order, then a butterfly: deterministic
    const int lane = threadIdx.x & 63;
    const int64_t pix = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pix >= pixels) return;
    const float* xp = x + pix * ld;
    const bool vec = (ld & 3) == 0 && (C & 7) == 0 && ((((uintptr_t)x) | ((uintptr_t)w) | ((uintptr_t)b)) & 15) == 0;
    float v[2][8];
    float s = 0.0f;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int c0 = r * 512 + lane * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[r][j] = 0.0f;
        if (c0 < C) {
            if (vec) {
                const f32x4 a = *(const f32x4*)(xp + c0), a2 = *(const f32x4*)(xp + c0 + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[r][j] = a[j], v[r][4 + j] = a2[j];
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (c0 + j < C) v[r][j] = xp[c0 + j];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[r][j];
        }
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)C;
    float q = 0.0f;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int c0 = r * 512 + lane * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (c0 + j < C) q += (v[r][j] - mean) * (v[r][j] - mean);
    }
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = 1.0f / sqrtf(q / (float)C + eps);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int c0 = r * 512 + lane * 8;
        if (c0 >= out.c) continue;
        bf16x8 oh, ol;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = c0 + j;
            const float y = c < C ? (v[r][j] - mean) * rstd * w[c] + b[c] : 0.0f;
            bf16_t hi, lo;
            split_bf16(y, hi, lo);
            oh[j] = hi;
            ol[j] = lo;
        }
        if (c0 + 8 <= out.c && (out.ld & 7) == 0 && ((((uintptr_t)out.hi) | ((uintptr_t)out.lo)) & 15) == 0) {
            *(bf16x8*)((bf16_t*)out.hi + pix * out.ld + c0) = oh;
            *(bf16x8*)((bf16_t*)out.lo + pix * out.ld + c0) = ol;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (c0 + j < out.c) {
                    ((bf16_t*)out.hi)[pix * out.ld + c0 + j] = oh[j];
                    ((bf16_t*)out.lo)[pix * out.ld + c0 + j] = ol[j];
                }
        }
    }
}

// GRN (convnext.py:37-48) on channel-last fp32 h [N*HW][ld]: Gx[n][c] = ||h[n, :, c]||_2 over the pixels; Nx = Gx / (mean_c Gx + 1e-6);
// out = gamma * (h * Nx) + beta + h.  Squares summed per pixel slice (part kernel), slices merged in order + the channel mean
// (one workgroup per sample), then the apply kernel.  Deterministic.
__global__ __launch_bounds__(256) void grn_part_kernel(const float* __restrict__ x, int ld, int HW, int C, int S, float* __restrict__ part) {
    __shared__ float red[32][33];
    const int n = blockIdx.y, c0 = blockIdx.x * 32, s = blockIdx.z;
    const int q = threadIdx.x & 7, row = threadIdx.x >> 3;                // thread = 4 channels (one 16-byte load) of every 32nd pixel of the slice
    const int c = c0 + 4 * q;
    const int chunk = (HW + S - 1) / S;
    const int p0 = s * chunk, p1 = (p0 + chunk < HW) ? p0 + chunk : HW;
    const float* xp = x + (int64_t)n * HW * ld + c;
    const bool vec = (ld & 3) == 0 && c + 4 <= C && (((uintptr_t)x) & 15) == 0;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int p = p0 + row; p < p1; p += 32) {
        float v[4];
        if (vec) {
            const f32x4 t = *(const f32x4*)(xp + (int64_t)p * ld);
            v[0] = t[0], v[1] = t[1], v[2] = t[2], v[3] = t[3];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (c + j < C) ? xp[(int64_t)p * ld + j] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += v[j] * v[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) red[row][4 * q + j] = acc[j];
    __syncthreads();
    if (threadIdx.x < 32 && c0 + (int)threadIdx.x < C) {
        float t = 0.0f;
        for (int r = 0; r < 32; ++r) t += red[r][threadIdx.x];
        part[((int64_t)n * S + s) * C + c0 + threadIdx.x] = t;
    }
}
__global__ __launch_bounds__(256) void grn_merge_kernel(const float* __restrict__ part, int C, int S, float* __restrict__ nx) {
    __shared__ float red[256];
    const int n = blockIdx.x;
    float local = 0.0f;
    for (int c = threadIdx.x; c < C; c += 256) {
        float t = 0.0f;
        const float* pp = part + (int64_t)n * S * C + c;
        for (int s0 = 0; s0 < S; s0 += 8) {      // 8 loads in flight, summed in slice order
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (s0 + j < S) ? pp[(int64_t)(s0 + j) * C] : 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (s0 + j < S) t += v[j];
        }
        const float g = sqrtf(t);
        nx[(int64_t)n * C + c] = g;
        local += g;
    }
    red[threadIdx.x] = local;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const float inv = 1.0f / (red[0] / (float)C + 1e-6f);
    for (int c = threadIdx.x; c < C; c += 256) nx[(int64_t)n * C + c] *= inv;
}
__global__ __launch_bounds__(256) void grn_apply_kernel(const float* __restrict__ x, int ld, const float* __restrict__ nx, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, ppms_sp out, int HW, int C, int64_t npix) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;          // one thread = one pixel x 8 channels
    const int groups = C >> 3;
    if (idx >= npix * groups) return;
    const int c0 = (int)(idx % groups) * 8;
    const int64_t p = idx / groups;
    const int64_t n = p / HW;
    bf16x8 oh, ol;
    float xv[8], nv[8], gv[8], bv[8];
    if ((ld & 3) == 0 && ((((uintptr_t)x) | ((uintptr_t)nx) | ((uintptr_t)gamma) | ((uintptr_t)beta)) & 15) == 0) {      // (C % 8 == 0: the host checks)
#pragma unroll
        for (int h4 = 0; h4 < 2; ++h4) {
            const f32x4 a = *(const f32x4*)(x + p * ld + c0 + 4 * h4), b4 = *(const f32x4*)(nx + n * C + c0 + 4 * h4);
            const f32x4 g4 = *(const f32x4*)(gamma + c0 + 4 * h4), e4 = *(const f32x4*)(beta + c0 + 4 * h4);
#pragma unroll
            for (int j = 0; j < 4; ++j) xv[4 * h4 + j] = a[j], nv[4 * h4 + j] = b4[j], gv[4 * h4 + j] = g4[j], bv[4 * h4 + j] = e4[j];
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e] = x[p * ld + c0 + e], nv[e] = nx[n * C + c0 + e], gv[e] = gamma[c0 + e], bv[e] = beta[c0 + e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float v = xv[e];
        const float y = gv[e] * (v * nv[e]) + bv[e] + v;
        bf16_t hh, ll;
        split_bf16(y, hh, ll);
        oh[e] = hh;
        ol[e] = ll;
    }
    const int64_t od = p * out.ld + c0;
    *(bf16x8*)((bf16_t*)out.hi + od) = oh;
    *(bf16x8*)((bf16_t*)out.lo + od) = ol;
}

}  // namespace

extern "C" int ppms_sp_upsample2(ppms_sp src, ppms_sp dst, int N, int H, int W, void* stream) {
    PPMS_REQUIRE(src.hi && src.lo && dst.hi && dst.lo && N > 0 && H > 0 && W > 0, "sp_upsample2: bad arguments");
    PPMS_REQUIRE(src.c % 8 == 0 && dst.c == src.c && src.ld % 8 == 0 && dst.ld % 8 == 0, "sp_upsample2: equal channel counts, multiples of 8");
    PPMS_REQUIRE((((uintptr_t)src.hi | (uintptr_t)src.lo | (uintptr_t)dst.hi | (uintptr_t)dst.lo) & 15) == 0, "sp_upsample2: views must be 16-B aligned");
    const int64_t npix = (int64_t)N * 4 * H * W;
    hipLaunchKernelGGL(sp_upsample2_kernel, dim3(ceil_div(npix * (src.c / 8), 256)), dim3(256), 0, (hipStream_t)stream, src, dst, H, W, npix);
    return ppms_check_launch("sp_upsample2");
}

extern "C" int ppms_dwconv(ppms_sp x, float* y, int ldy, const float* w, const float* b, int k, int N, int H, int W, void* stream) {
    PPMS_REQUIRE(x.hi && x.lo && y && w && b && N > 0 && H > 0 && W > 0 && k == 7, "dwconv: bad arguments (k = 7: ConvNeXt's depthwise kernel)");
    PPMS_REQUIRE(x.c % 8 == 0 && x.ld % 8 == 0 && ldy >= x.c && ldy % 4 == 0 && (((uintptr_t)x.hi | (uintptr_t)x.lo | (uintptr_t)y | (uintptr_t)b) & 15) == 0,
                 "dwconv: channel counts multiples of 8, 16-B aligned operands");
    const int64_t rows = (int64_t)N * H;
    const int cblocks = (int)ceil_div(x.c, 64);
    const int64_t per_block = rows * ((W + DWP_PX - 1) / DWP_PX) * 8;       // threads of a full 64-channel block
    hipLaunchKernelGGL(dwconv_plain_kernel, dim3(ceil_div(per_block, 256), cblocks), dim3(256), 0, (hipStream_t)stream, x, y, ldy, w, b, H, W, rows);
    return ppms_check_launch("dwconv");
}

extern "C" int ppms_layernorm_any(const float* x, int ld, const float* w, const float* b, float eps, ppms_sp out, int64_t pixels, int C, void* stream) {
    PPMS_REQUIRE(x && w && b && out.hi && out.lo && pixels > 0 && C > 0 && ld >= C && out.c >= C && eps > 0.0f, "layernorm_any: bad arguments");
    PPMS_REQUIRE(out.c <= 1024, "layernorm_any: at most 1024 channels (got %d)", out.c);
    hipLaunchKernelGGL(layernorm_any_kernel, dim3(ceil_div(pixels, 4)), dim3(256), 0, (hipStream_t)stream, x, ld, w, b, eps, out, pixels, C);
    return ppms_check_launch("layernorm_any");
}

extern "C" int64_t ppms_grn_workspace_bytes(int N, int HW, int C) {
    if (N <= 0 || HW <= 0 || C <= 0) return 0;
    return ((int64_t)N * in_slices_host(N, HW, C) * C + (int64_t)N * C) * 4;
}

extern "C" int ppms_grn(const float* x, int ld, const float* gamma, const float* beta, ppms_sp out, int N, int HW, int C, void* workspace, void* stream) {
    PPMS_REQUIRE(x && gamma && beta && out.hi && out.lo && workspace && N > 0 && HW > 0 && C > 0 && C % 8 == 0 && ld >= C, "grn: bad arguments");
    PPMS_REQUIRE(out.c >= C && out.ld % 8 == 0 && (((uintptr_t)out.hi | (uintptr_t)out.lo) & 15) == 0, "grn: output view must cover C channels, 16-B aligned");
    const int S = in_slices_host(N, HW, C);
    float* part = (float*)workspace;
    float* nx = part + (size_t)N * S * C;
    hipLaunchKernelGGL(grn_part_kernel, dim3(ceil_div(C, 32), N, S), dim3(256), 0, (hipStream_t)stream, x, ld, HW, C, S, part);
    hipLaunchKernelGGL(grn_merge_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, (const float*)part, C, S, nx);
    const int64_t npix = (int64_t)N * HW;
    hipLaunchKernelGGL(grn_apply_kernel, dim3(ceil_div(npix * (C / 8), 256)), dim3(256), 0, (hipStream_t)stream, x, ld, (const float*)nx, gamma, beta, out, HW,
                       C, npix);
    return ppms_check_launch("grn");
}

extern "C" int ppms_img_s2d(const float* img, ppms_sp dst, int N, int C, int H, int W, int k, void* stream) {
    PPMS_REQUIRE(img && dst.hi && dst.lo && N > 0 && C > 0 && H > 0 && W > 0 && (k == 2 || k == 4), "img_s2d: bad arguments (k = 2 or 4)");
    PPMS_REQUIRE(H % k == 0 && W % k == 0, "img_s2d: H = %d, W = %d must be multiples of %d", H, W, k);
    PPMS_REQUIRE(dst.c >= k * k * C && dst.c % 8 == 0 && dst.ld % 8 == 0 && (((uintptr_t)dst.hi | (uintptr_t)dst.lo) & 15) == 0,
                 "img_s2d: destination view needs >= %d channels, multiples of 8, 16-B aligned", k * k * C);
    const int64_t npix = (int64_t)N * (H / k) * (W / k);
    hipLaunchKernelGGL(img_s2d_kernel, dim3(ceil_div(npix * (dst.c / 8), 256)), dim3(256), 0, (hipStream_t)stream, img, dst, C, H, W, k, npix);
    return ppms_check_launch("img_s2d");
}

// what both video ingest entry points check about sizes, pads, table and destinations, and their launch (`who` names the entry point)
template <class Source>
static int video_ingest_launch(const char* who, const Source& source, int N, int H0, int W0, int pad_left, int pad_top, int H, int W, const float* lut,
                               ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream) {
    PPMS_REQUIRE(lut, "%s: null table pointer", who);
    PPMS_REQUIRE(N > 0 && H0 > 0 && W0 > 0 && H > 0 && W > 0, "%s: N = %d, H0 = %d, W0 = %d, H = %d, W = %d must be positive", who, N, H0, W0, H, W);
    PPMS_REQUIRE(H % 4 == 0 && W % 4 == 0, "%s: H = %d, W = %d must be multiples of 4", who, H, W);
    PPMS_REQUIRE(pad_left >= 0 && pad_top >= 0 && (int64_t)pad_top + H0 <= H && (int64_t)pad_left + W0 <= W,
                 "%s: pad_left = %d, pad_top = %d with a %d x %d source do not fit the %d x %d padded image", who, pad_left, pad_top, H0, W0, H, W);
    PPMS_REQUIRE(dst_fnet.hi || dst_cnet.hi, "%s: both destinations skipped", who);
    const ppms_sp* dsts[2] = {&dst_fnet, &dst_cnet};
    int64_t threads[2] = {0, 0};
    for (int s = 0; s < 2; ++s) {
        const ppms_sp& d = *dsts[s];
        if (!d.hi) continue;                                               // skipped
        const int k = s == 0 ? 2 : 4;
        PPMS_REQUIRE(d.lo && d.c >= k * k * 3 && d.c % 8 == 0 && d.ld % 8 == 0 && d.ld >= d.c && (((uintptr_t)d.hi | (uintptr_t)d.lo) & 15) == 0,
                     "%s: the k = %d destination view needs >= %d channels, multiples of 8, 16-B aligned", who, k, k * k * 3);
        threads[s] = (int64_t)(s == 0 ? 2 : 1) * N * (H / k) * (W / k) * (d.c / 8);
    }
    const int64_t total = threads[0] + threads[1];
    PPMS_REQUIRE((total + 255) / 256 <= 0x7fffffff, "%s: %lld threads exceed one grid", who, (long long)total);
    size_t table_bytes = 0;                                                // dynamic LDS: the level table of a source that sizes it by depth
    if constexpr (Source::table_by_depth) table_bytes = sizeof(float) * (size_t)source.levels();
    hipLaunchKernelGGL(video_ingest_kernel<Source>, dim3(ceil_div(total, 256)), dim3(256), table_bytes, (hipStream_t)stream, source, N, H0, W0, pad_left, pad_top, H, W,
                       lut, dst_fnet, dst_cnet, threads[0], total);
    return ppms_check_launch(who);
}

extern "C" int ppms_video_ingest_u8(const uint8_t* left, const uint8_t* right, int64_t frame_stride, int N, int H0, int W0, int pad_left, int pad_top, int H,
                                    int W, const float* lut, ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream) {
    PPMS_REQUIRE(left && right, "video_ingest_u8: null source pointer");
    PPMS_REQUIRE(frame_stride >= (int64_t)3 * H0 * W0, "video_ingest_u8: frame_stride = %lld is less than a frame's 3 * H0 * W0 bytes", (long long)frame_stride);
    return video_ingest_launch("video_ingest_u8", rgb_planes_source{left, right, frame_stride, N, H0, W0}, N, H0, W0, pad_left, pad_top, H, W, lut, dst_fnet,
                               dst_cnet, stream);
}

extern "C" int ppms_yuv_struct_sizes(int* view, int* matrix) {
    if (view) *view = (int)sizeof(ppms_yuv_view);
    if (matrix) *matrix = (int)sizeof(ppms_yuv_matrix);
    return PPMS_OK;
}

// what both YUV entry points check about the views (frames of H0 x W0, named `hname` x `wname` in the messages) and the matrix
static int yuv420_check(const char* who, const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, const float* lut, int N, int H0,
                        int W0, const char* hname, const char* wname) {
    PPMS_REQUIRE(left && right && m && lut, "%s: null view, matrix or table pointer", who);
    PPMS_REQUIRE(N > 0 && H0 > 0 && W0 > 0, "%s: N = %d, %s = %d, %s = %d must be positive", who, N, hname, H0, wname, W0);
    const int Hc = (H0 + 1) / 2, Wc = (W0 + 1) / 2;                        // chroma planes: ceil(H0 / 2) x ceil(W0 / 2)
    const ppms_yuv_view* views[2] = {left, right};
    for (int s = 0; s < 2; ++s) {
        const ppms_yuv_view& v = *views[s];
        const char* side = s == 0 ? "left" : "right";
        PPMS_REQUIRE(v.y && v.u && v.v, "%s: null plane pointer in the %s view", who, side);
        PPMS_REQUIRE(v.step_c == 1 || v.step_c == 2, "%s: %s step_c = %d must be 1 (planar) or 2 (interleaved)", who, side, v.step_c);
        PPMS_REQUIRE(v.reserved == 0, "%s: %s view: reserved = %d must be 0", who, side, v.reserved);
        const int64_t row_c = (int64_t)v.step_c * (Wc - 1) + 1;            // bytes from a chroma row's first sample to its last
        PPMS_REQUIRE(v.pitch_y >= W0, "%s: %s pitch_y = %d is less than %s = %d", who, side, v.pitch_y, wname, W0);
        PPMS_REQUIRE(v.pitch_c >= row_c, "%s: %s pitch_c = %d is less than a chroma row's %lld bytes", who, side, v.pitch_c, (long long)row_c);
        PPMS_REQUIRE(v.frame_stride_y >= (int64_t)(H0 - 1) * v.pitch_y + W0, "%s: %s frame_stride_y = %lld is less than a luma plane", who, side,
                     (long long)v.frame_stride_y);
        PPMS_REQUIRE(v.frame_stride_c >= (int64_t)(Hc - 1) * v.pitch_c + row_c, "%s: %s frame_stride_c = %lld is less than a chroma plane", who, side,
                     (long long)v.frame_stride_c);
    }
    PPMS_REQUIRE(m->shift >= 8 && m->shift <= 20, "%s: shift = %d must lie in [8, 20]", who, m->shift);
    PPMS_REQUIRE(m->reserved == 0, "%s: matrix: reserved = %d must be 0", who, m->reserved);
    // coefficients below 4.0 keep every sum of the conversion inside 32 bits: 2^22 (255 + 128 + 128) + 2^19 < 2^31 at shift = 20
    const int32_t lim = 4 << m->shift;
    PPMS_REQUIRE(m->y_off >= 0 && m->y_off <= 255 && m->cy >= 0 && m->cy < lim && m->crv >= 0 && m->crv < lim && m->cgu >= 0 && m->cgu < lim && m->cgv >= 0 &&
                     m->cgv < lim && m->cbu >= 0 && m->cbu < lim,
                 "%s: y_off must lie in [0, 255] and every coefficient in [0, 4 << shift)", who);
    return PPMS_OK;
}

extern "C" int ppms_video_ingest_yuv420(const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, int N, int H0, int W0, int pad_left,
                                        int pad_top, int H, int W, const float* lut, ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream) {
    if (const int rc = yuv420_check("video_ingest_yuv420", left, right, m, lut, N, H0, W0, "H0", "W0")) return rc;
    return video_ingest_launch("video_ingest_yuv420", yuv420_source{*left, *right, *m, N}, N, H0, W0, pad_left, pad_top, H, W, lut, dst_fnet, dst_cnet, stream);
}

extern "C" int ppms_yuv_format_struct_size(int* fmt) {
    if (fmt) *fmt = (int)sizeof(ppms_yuv_format);
    return PPMS_OK;
}

// what both ppms_video_ingest_yuv entry points check about the format, the views (frames of H0 x W0, named `hname` x `wname` in the messages)
// and the matrix: everything yuv420_check refuses, restated for `sample_bytes`-wide samples of `depth` bits and the format's subsampling
static int yuv_check(const char* who, const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, const ppms_yuv_format* fmt,
                     const float* lut, int N, int H0, int W0, const char* hname, const char* wname) {
    PPMS_REQUIRE(left && right && m && fmt && lut, "%s: null view, matrix, format or table pointer", who);
    PPMS_REQUIRE(N > 0 && H0 > 0 && W0 > 0, "%s: N = %d, %s = %d, %s = %d must be positive", who, N, hname, H0, wname, W0);
    const ppms_yuv_format& f = *fmt;
    const int sb = f.sample_bytes;
    PPMS_REQUIRE(sb == 1 || sb == 2, "%s: sample_bytes = %d must be 1 or 2", who, sb);
    PPMS_REQUIRE(sb == 1 ? f.depth == 8 : (f.depth == 10 || f.depth == 12),
                 "%s: depth = %d does not go with sample_bytes = %d (8 with 1; 10 or 12 with 2)", who, f.depth, sb);
    PPMS_REQUIRE(f.lsb == 0 || (sb == 2 && f.lsb == 16 - f.depth), "%s: lsb = %d must be 0, or 16 - depth for 16-bit words", who, f.lsb);
    PPMS_REQUIRE((f.sub_x == 1 && f.sub_y == 1) || (f.sub_x == 1 && f.sub_y == 0) || (f.sub_x == 0 && f.sub_y == 0),
                 "%s: sub_x = %d, sub_y = %d must be (1, 1) 4:2:0, (1, 0) 4:2:2 or (0, 0) 4:4:4", who, f.sub_x, f.sub_y);
    PPMS_REQUIRE(f.reserved[0] == 0 && f.reserved[1] == 0 && f.reserved[2] == 0, "%s: format: reserved must be 0", who);
    const int Hc = (H0 + (1 << f.sub_y) - 1) >> f.sub_y, Wc = (W0 + (1 << f.sub_x) - 1) >> f.sub_x;      // chroma planes: ceil(H0 / 2^sub_y) x ceil(W0 / 2^sub_x)
    const ppms_yuv_view* views[2] = {left, right};
    for (int s = 0; s < 2; ++s) {
        const ppms_yuv_view& v = *views[s];
        const char* side = s == 0 ? "left" : "right";
        PPMS_REQUIRE(v.y && v.u && v.v, "%s: null plane pointer in the %s view", who, side);
        PPMS_REQUIRE(v.step_c == sb || v.step_c == 2 * sb, "%s: %s step_c = %d must be %d (planar) or %d (interleaved)", who, side, v.step_c, sb, 2 * sb);
        PPMS_REQUIRE(v.reserved == 0, "%s: %s view: reserved = %d must be 0", who, side, v.reserved);
        if (sb == 2)
            PPMS_REQUIRE((((uintptr_t)v.y | (uintptr_t)v.u | (uintptr_t)v.v | (uintptr_t)v.frame_stride_y | (uintptr_t)v.frame_stride_c | (uintptr_t)v.pitch_y |
                           (uintptr_t)v.pitch_c) & 1) == 0,
                         "%s: %s view: an odd pointer or stride; 16-bit samples need even pointers, pitches and frame strides", who, side);
        const int64_t row_y = (int64_t)W0 * sb, row_c = (int64_t)v.step_c * (Wc - 1) + sb;     // bytes from a row's first sample to the end of its last
        PPMS_REQUIRE(v.pitch_y >= row_y, "%s: %s pitch_y = %d is less than a luma row's %lld bytes (%s = %d)", who, side, v.pitch_y, (long long)row_y, wname, W0);
        PPMS_REQUIRE(v.pitch_c >= row_c, "%s: %s pitch_c = %d is less than a chroma row's %lld bytes", who, side, v.pitch_c, (long long)row_c);
        PPMS_REQUIRE(v.frame_stride_y >= (int64_t)(H0 - 1) * v.pitch_y + row_y, "%s: %s frame_stride_y = %lld is less than a luma plane", who, side,
                     (long long)v.frame_stride_y);
        PPMS_REQUIRE(v.frame_stride_c >= (int64_t)(Hc - 1) * v.pitch_c + row_c, "%s: %s frame_stride_c = %lld is less than a chroma plane", who, side,
                     (long long)v.frame_stride_c);
    }
    PPMS_REQUIRE(m->shift >= 8 && m->shift <= 26 - f.depth, "%s: shift = %d must lie in [8, %d] at depth %d", who, m->shift, 26 - f.depth, f.depth);
    PPMS_REQUIRE(m->reserved == 0, "%s: matrix: reserved = %d must be 0", who, m->reserved);
    // coefficients below 4.0 keep every sum of the conversion inside 32 bits: three terms below 4 * 2^shift * 2^depth <= 2^28 each, plus 2^(shift - 1)
    const int32_t lim = 4 << m->shift;
    PPMS_REQUIRE(m->y_off >= 0 && m->y_off < (1 << f.depth) && m->cy >= 0 && m->cy < lim && m->crv >= 0 && m->crv < lim && m->cgu >= 0 && m->cgu < lim &&
                     m->cgv >= 0 && m->cgv < lim && m->cbu >= 0 && m->cbu < lim,
                 "%s: y_off must lie in [0, %d] and every coefficient in [0, 4 << shift)", who, (1 << f.depth) - 1);
    return PPMS_OK;
}

template <class T>
static yuv_source<T> make_yuv_source(const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, const ppms_yuv_format* f, int N) {
    return yuv_source<T>{*left, *right, *m, N, f->depth, f->lsb, f->sub_x, f->sub_y};
}

extern "C" int ppms_video_ingest_yuv(const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, const ppms_yuv_format* fmt, int N, int H0,
                                     int W0, int pad_left, int pad_top, int H, int W, const float* lut, ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream) {
    const char* who = "video_ingest_yuv";
    if (const int rc = yuv_check(who, left, right, m, fmt, lut, N, H0, W0, "H0", "W0")) return rc;
    if (fmt->sample_bytes == 1)
        return video_ingest_launch(who, make_yuv_source<uint8_t>(left, right, m, fmt, N), N, H0, W0, pad_left, pad_top, H, W, lut, dst_fnet, dst_cnet, stream);
    return video_ingest_launch(who, make_yuv_source<uint16_t>(left, right, m, fmt, N), N, H0, W0, pad_left, pad_top, H, W, lut, dst_fnet, dst_cnet, stream);
}

extern "C" int ppms_remap_struct_size(int* view) {
    if (view) *view = (int)sizeof(ppms_remap_view);
    return PPMS_OK;
}

// what the remap entry points check about the two maps of a W0 columns wide rectified frame (`fill_max`: the top level of the source's samples)
static int remap_check(const char* who, const ppms_remap_view* lmap, const ppms_remap_view* rmap, int W0, int fill_max = 255) {
    PPMS_REQUIRE(lmap && rmap, "%s: null map pointer (lmap, rmap)", who);
    const ppms_remap_view* maps[2] = {lmap, rmap};
    for (int s = 0; s < 2; ++s) {
        const ppms_remap_view& v = *maps[s];
        const char* side = s == 0 ? "lmap" : "rmap";
        PPMS_REQUIRE(v.xy && v.frac, "%s: null xy or frac pointer in %s", who, side);
        PPMS_REQUIRE(v.pitch >= W0, "%s: %s pitch = %d is less than W0 = %d", who, side, v.pitch, W0);
        PPMS_REQUIRE(v.hs >= 1 && v.hs <= 32768 && v.ws >= 1 && v.ws <= 32768, "%s: %s source frame hs = %d, ws = %d must lie in [1, 32768]", who, side,
                     v.hs, v.ws);
        PPMS_REQUIRE(v.border == 0 || v.border == 1, "%s: %s border = %d must be 0 (replicate) or 1 (constant)", who, side, v.border);
        PPMS_REQUIRE(v.fill >= 0 && v.fill <= fill_max, "%s: %s fill = %d must lie in [0, %d]", who, side, v.fill, fill_max);
        PPMS_REQUIRE(v.reserved == 0, "%s: %s reserved = %d must be 0", who, side, v.reserved);
        PPMS_REQUIRE(((uintptr_t)v.xy & 3) == 0 && ((uintptr_t)v.frac & 1) == 0, "%s: %s misaligned pointer: xy needs 4 bytes, frac 2", who, side);
    }
    PPMS_REQUIRE(lmap->hs == rmap->hs && lmap->ws == rmap->ws, "%s: lmap and rmap differ in hs, ws: %d x %d and %d x %d", who, lmap->hs, lmap->ws, rmap->hs,
                 rmap->ws);
    return PPMS_OK;
}

extern "C" int ppms_video_ingest_u8_remap(const uint8_t* left, const uint8_t* right, int64_t frame_stride, const ppms_remap_view* lmap,
                                          const ppms_remap_view* rmap, int N, int H0, int W0, int pad_left, int pad_top, int H, int W, const float* lut,
                                          ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream) {
    const char* who = "video_ingest_u8_remap";
    PPMS_REQUIRE(left && right, "%s: null source pointer", who);
    if (const int rc = remap_check(who, lmap, rmap, W0)) return rc;
    const int hs = lmap->hs, ws = lmap->ws;
    PPMS_REQUIRE(frame_stride >= (int64_t)3 * hs * ws, "%s: frame_stride = %lld is less than a source frame's 3 * hs * ws bytes", who, (long long)frame_stride);
    const remapped_source<rgb_planes_source> source{rgb_planes_source{left, right, frame_stride, N, hs, ws}, *lmap, *rmap, N};
    return video_ingest_launch(who, source, N, H0, W0, pad_left, pad_top, H, W, lut, dst_fnet, dst_cnet, stream);
}

extern "C" int ppms_video_ingest_yuv420_remap(const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, const ppms_remap_view* lmap,
                                              const ppms_remap_view* rmap, int N, int H0, int W0, int pad_left, int pad_top, int H, int W, const float* lut,
                                              ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream) {
    const char* who = "video_ingest_yuv420_remap";
    if (const int rc = remap_check(who, lmap, rmap, W0)) return rc;
    if (const int rc = yuv420_check(who, left, right, m, lut, N, lmap->hs, lmap->ws, "hs", "ws")) return rc;
    const remapped_source<yuv420_source> source{yuv420_source{*left, *right, *m, N}, *lmap, *rmap, N};
    return video_ingest_launch(who, source, N, H0, W0, pad_left, pad_top, H, W, lut, dst_fnet, dst_cnet, stream);
}

extern "C" int ppms_video_ingest_yuv_remap(const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, const ppms_yuv_format* fmt,
                                           const ppms_remap_view* lmap, const ppms_remap_view* rmap, int N, int H0, int W0, int pad_left, int pad_top, int H,
                                           int W, const float* lut, ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream) {
    const char* who = "video_ingest_yuv_remap";
    // `fill` is a level of the format's depth (a format that names no depth is refused right behind the maps, which bound hs and ws for that check)
    const int top = fmt && (fmt->depth == 10 || fmt->depth == 12) ? (1 << fmt->depth) - 1 : 255;
    if (const int rc = remap_check(who, lmap, rmap, W0, top)) return rc;
    if (const int rc = yuv_check(who, left, right, m, fmt, lut, N, lmap->hs, lmap->ws, "hs", "ws")) return rc;
    if (fmt->sample_bytes == 1) {
        const remapped_source<yuv_source<uint8_t>> source{make_yuv_source<uint8_t>(left, right, m, fmt, N), *lmap, *rmap, N};
        return video_ingest_launch(who, source, N, H0, W0, pad_left, pad_top, H, W, lut, dst_fnet, dst_cnet, stream);
    }
    const remapped_source<yuv_source<uint16_t>> source{make_yuv_source<uint16_t>(left, right, m, fmt, N), *lmap, *rmap, N};
    return video_ingest_launch(who, source, N, H0, W0, pad_left, pad_top, H, W, lut, dst_fnet, dst_cnet, stream);
}

extern "C" int ppms_raw_struct_sizes(int* view, int* format) {
    if (view) *view = (int)sizeof(ppms_raw_view);
    if (format) *format = (int)sizeof(ppms_raw_format);
    return PPMS_OK;
}

// what both ppms_video_ingest_raw entry points check about the format and the views (frames of H0 x W0, named `hname` x `wname` in the messages)
static int raw_check(const char* who, const ppms_raw_view* left, const ppms_raw_view* right, const ppms_raw_format* fmt, const float* lut, int N, int H0,
                     int W0, const char* hname, const char* wname) {
    PPMS_REQUIRE(left && right && fmt && lut, "%s: null view, format or table pointer", who);
    PPMS_REQUIRE(N > 0 && H0 > 0 && W0 > 0, "%s: N = %d, %s = %d, %s = %d must be positive", who, N, hname, H0, wname, W0);
    const ppms_raw_format& f = *fmt;
    const int sb = f.sample_bytes;
    PPMS_REQUIRE(sb == 1 || sb == 2, "%s: sample_bytes = %d must be 1 or 2", who, sb);
    PPMS_REQUIRE(sb == 1 ? f.depth == 8 : (f.depth == 10 || f.depth == 12),
                 "%s: depth = %d does not go with sample_bytes = %d (8 with 1; 10 or 12 with 2)", who, f.depth, sb);
    PPMS_REQUIRE(f.lsb == 0 || (sb == 2 && f.lsb == 16 - f.depth), "%s: lsb = %d must be 0, or 16 - depth for 16-bit words", who, f.lsb);
    PPMS_REQUIRE(f.pattern >= 0 && f.pattern <= 4, "%s: pattern = %d must be 0 (RGGB), 1 (BGGR), 2 (GRBG), 3 (GBRG) or 4 (MONO)", who, f.pattern);
    PPMS_REQUIRE(f.black >= 0 && f.black < (1 << f.depth), "%s: black = %d must lie in [0, %d]", who, f.black, (1 << f.depth) - 1);
    PPMS_REQUIRE(f.shift >= 4 && f.shift <= 14, "%s: shift = %d must lie in [4, 14]", who, f.shift);
    // gains below 16.0 keep every sum inside 32 bits: 2^12 * 2^18 + 2^13 < 2^31 at depth 12 and shift = 14
    const int32_t lim = 16 << f.shift;
    PPMS_REQUIRE(f.gain[0] >= 0 && f.gain[0] < lim && f.gain[1] >= 0 && f.gain[1] < lim && f.gain[2] >= 0 && f.gain[2] < lim,
                 "%s: every gain must lie in [0, 16 << shift)", who);
    PPMS_REQUIRE(f.reserved[0] == 0 && f.reserved[1] == 0 && f.reserved[2] == 0, "%s: format: reserved must be 0", who);
    PPMS_REQUIRE(f.pattern == 4 || (H0 >= 2 && W0 >= 2), "%s: a colour pattern needs a frame of at least 2 x 2, got %s = %d, %s = %d", who, hname, H0, wname, W0);
    const ppms_raw_view* views[2] = {left, right};
    for (int s = 0; s < 2; ++s) {
        const ppms_raw_view& v = *views[s];
        const char* side = s == 0 ? "left" : "right";
        PPMS_REQUIRE(v.data, "%s: null data pointer in the %s view", who, side);
        PPMS_REQUIRE(v.reserved == 0, "%s: %s view: reserved = %d must be 0", who, side, v.reserved);
        if (sb == 2)
            PPMS_REQUIRE((((uintptr_t)v.data | (uintptr_t)v.frame_stride | (uintptr_t)v.pitch) & 1) == 0,
                         "%s: %s view: an odd pointer or stride; 16-bit samples need even pointers, pitches and frame strides", who, side);
        const int64_t row = (int64_t)W0 * sb;                              // bytes from a row's first sample to the end of its last
        PPMS_REQUIRE(v.pitch >= row, "%s: %s pitch = %d is less than a row's %lld bytes (%s = %d)", who, side, v.pitch, (long long)row, wname, W0);
        PPMS_REQUIRE(N == 1 || v.frame_stride >= (int64_t)(H0 - 1) * v.pitch + row, "%s: %s frame_stride = %lld is less than a frame", who, side,
                     (long long)v.frame_stride);
    }
    return PPMS_OK;
}

template <class T>
static raw_source<T> make_raw_source(const ppms_raw_view* left, const ppms_raw_view* right, const ppms_raw_format* f, int N, int hs, int ws) {
    return raw_source<T>{*left, *right, N, hs, ws, f->depth, f->lsb, f->pattern, f->black, f->gain[0], f->gain[1], f->gain[2], f->shift};
}

extern "C" int ppms_video_ingest_raw(const ppms_raw_view* left, const ppms_raw_view* right, const ppms_raw_format* fmt, int N, int H0, int W0, int pad_left,
                                     int pad_top, int H, int W, const float* lut, ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream) {
    const char* who = "video_ingest_raw";
    if (const int rc = raw_check(who, left, right, fmt, lut, N, H0, W0, "H0", "W0")) return rc;
    if (fmt->sample_bytes == 1)
        return video_ingest_launch(who, make_raw_source<uint8_t>(left, right, fmt, N, H0, W0), N, H0, W0, pad_left, pad_top, H, W, lut, dst_fnet, dst_cnet, stream);
    return video_ingest_launch(who, make_raw_source<uint16_t>(left, right, fmt, N, H0, W0), N, H0, W0, pad_left, pad_top, H, W, lut, dst_fnet, dst_cnet, stream);
}

extern "C" int ppms_video_ingest_raw_remap(const ppms_raw_view* left, const ppms_raw_view* right, const ppms_raw_format* fmt, const ppms_remap_view* lmap,
                                           const ppms_remap_view* rmap, int N, int H0, int W0, int pad_left, int pad_top, int H, int W, const float* lut,
                                           ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream) {
    const char* who = "video_ingest_raw_remap";
    // `fill` is a level of the format's depth (a format that names no depth is refused right behind the maps, which bound hs and ws for that check)
    const int top = fmt && (fmt->depth == 10 || fmt->depth == 12) ? (1 << fmt->depth) - 1 : 255;
    if (const int rc = remap_check(who, lmap, rmap, W0, top)) return rc;
    const int hs = lmap->hs, ws = lmap->ws;
    if (const int rc = raw_check(who, left, right, fmt, lut, N, hs, ws, "hs", "ws")) return rc;
    if (fmt->sample_bytes == 1) {
        const remapped_source<raw_source<uint8_t>> source{make_raw_source<uint8_t>(left, right, fmt, N, hs, ws), *lmap, *rmap, N};
        return video_ingest_launch(who, source, N, H0, W0, pad_left, pad_top, H, W, lut, dst_fnet, dst_cnet, stream);
    }
    const remapped_source<raw_source<uint16_t>> source{make_raw_source<uint16_t>(left, right, fmt, N, hs, ws), *lmap, *rmap, N};
    return video_ingest_launch(who, source, N, H0, W0, pad_left, pad_top, H, W, lut, dst_fnet, dst_cnet, stream);
}

extern "C" int ppms_sp_s2d(ppms_sp src, ppms_sp dst, int N, int H, int W, void* stream) {
    PPMS_REQUIRE(src.hi && src.lo && dst.hi && dst.lo && N > 0 && H > 0 && W > 0, "sp_s2d: bad arguments");
    PPMS_REQUIRE(H % 2 == 0 && W % 2 == 0, "sp_s2d: H = %d, W = %d must be even", H, W);
    PPMS_REQUIRE(src.c % 8 == 0 && dst.c == 4 * src.c && src.ld % 8 == 0 && dst.ld % 8 == 0, "sp_s2d: dst must have 4x the channels of src (multiples of 8)");
    PPMS_REQUIRE((((uintptr_t)src.hi | (uintptr_t)src.lo | (uintptr_t)dst.hi | (uintptr_t)dst.lo) & 15) == 0, "sp_s2d: views must be 16-B aligned");
    const int64_t npix = (int64_t)N * (H / 2) * (W / 2);
    hipLaunchKernelGGL(sp_s2d_kernel, dim3(ceil_div(npix * (dst.c / 8), 256)), dim3(256), 0, (hipStream_t)stream, src, dst, H, W, npix);
    return ppms_check_launch("sp_s2d");
}

extern "C" int64_t ppms_instnorm_workspace_bytes(int N, int HW, int C) {
    if (N <= 0 || HW <= 0 || C <= 0) return 0;
    return (int64_t)N * in_slices_host(N, HW, C) * C * 4 * 4;             // one 16-byte record (m_s, M2_s, r_s, -) per (n, slice, c)
}

extern "C" int ppms_instnorm_stats(const float* x, int ld, int N, int HW, int C, float eps, float* stats, void* workspace, void* stream) {
    PPMS_REQUIRE(x && stats && workspace && N > 0 && HW > 0 && C > 0 && ld >= C && eps > 0.0f, "instnorm_stats: bad arguments");
    PPMS_REQUIRE(((uintptr_t)workspace & 15) == 0, "instnorm_stats: the workspace must be 16-B aligned");
    const int S = in_slices_host(N, HW, C);
    hipLaunchKernelGGL(instnorm_part_kernel, dim3(ceil_div(C, 32), N, S), dim3(256), 0, (hipStream_t)stream, x, ld, HW, C, S, (float*)workspace);
    hipLaunchKernelGGL(instnorm_merge_kernel, dim3(ceil_div(N * C, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, HW, C, S, eps, N * C,
                       stats);
    return ppms_check_launch("instnorm_stats");
}

extern "C" int ppms_instnorm_apply(const float* x, int ld, const float* stats, ppms_sp res, int relu, ppms_sp out, int N, int HW, int C, void* stream) {
    PPMS_REQUIRE(x && stats && out.hi && out.lo && N > 0 && HW > 0 && C > 0 && ld >= C, "instnorm_apply: bad arguments");
    PPMS_REQUIRE(out.c >= C && out.c % 8 == 0 && out.ld % 8 == 0 && (((uintptr_t)out.hi | (uintptr_t)out.lo) & 15) == 0,
                 "instnorm_apply: output view needs >= %d channels, multiples of 8, 16-B aligned", C);
    PPMS_REQUIRE(res.hi == nullptr || (res.lo && res.c >= ((C + 7) / 8) * 8 && res.ld % 8 == 0 && (((uintptr_t)res.hi | (uintptr_t)res.lo) & 15) == 0),
                 "instnorm_apply: residual view must cover the normalised channels (multiples of 8, 16-B aligned)");
    const int64_t npix = (int64_t)N * HW;
    hipLaunchKernelGGL(instnorm_apply_kernel, dim3(ceil_div(npix * (out.c / 8), 256)), dim3(256), 0, (hipStream_t)stream, x, ld, stats, res, relu, out, HW, C,
                       npix);
    return ppms_check_launch("instnorm_apply");
}
