// The video doors of the C ABI (include/ppms.h: ppms_video_ingest_*): decoded or raw stereo video -> the first-layer operands of both encoders.
// One kernel template over a Source, one check-and-launch path on the host.  Colour out (ppms_video_colour_*) is a second kernel template over the
// same Sources behind the same doors and checks: the left view as 4-byte pixels (its plane's check: egress_shared.h).
#include "egress_shared.h"

namespace {

// decoded video -> the first-layer operands of both encoders in one launch (ppms_video_ingest_u8 / ppms_video_ingest_yuv420 / ppms_video_ingest_yuv / ppms_video_ingest_raw
// and the packed doors ppms_video_ingest_yuv_packed / ppms_video_ingest_raw_packed / ppms_video_ingest_rgb_packed):
// what normalisation (a table the caller built with the float path's own torch expression: 256 entries, or 1 << depth for a source whose
// table_by_depth is true, which also answers levels()), replicate padding (clamped source
// coordinate), torch.cat([left, right]) and the two img_s2d launches produce from the fp32 images.  Thread = one output pixel x 8 channels
// of one destination, as in img_s2d_kernel (encoder_ops.hip): indices [0, nf) serve the k = 2 operand of the 2 N images (left frames, then right frames),
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

// packed 4:2:2 (ppms_video_ingest_yuv_packed): one pitched surface per view whose rows are streams of components.  Column x of the view is
// surface column p = x + x0 (x0 even: the host refuses a split chroma pair), its pair j = p >> 1, and with `order` yuyv | uyvy | yvyu | vyuy the
// components are Y = 2 p + a, U = 4 j + b, V = 4 j + c for (a, b, c) = (0, 1, 3), (1, 0, 2), (0, 3, 1), (1, 2, 0): a = order & 1,
// b = 1 - a + (order & 2), c = 3 - order.  Container says where component i lies: 0 byte i, 1 little-endian 16-bit word i, (word >> lsb) masked to
// `depth` bits, 2 (v210) bits [10 (i % 3), 10 (i % 3) + 10) of 32-bit word i / 3.  Loads are of one container element (the host checks the
// alignment of pointers and strides for 16- and 32-bit elements).  (y, x) arrives clamped into the hs x ws frame, so p <= P - 1 with P = x0 + ws,
// and the largest component index is that of the last pair, 4 ceil(P / 2) - 1: inside the 4 ceil(P / 2) bytes, 8 ceil(P / 2) bytes or -- 12 components
// to 16 bytes -- 16 ceil(P / 6) bytes the host demands of the pitch.  No load leaves [row, row + row_bytes).  From the three samples on it is yuv_source's
// conversion, restated (a helper shared with yuv_source changed the schedule of its four kernels; they keep their code).
template <int Container>
struct yuv_packed_source {
    ppms_packed_view left, right;
    ppms_yuv_matrix mat;
    int N, depth, lsb, order;                                             // uniform: the ppms_yuv_packed_format
    static constexpr bool table_by_depth = true;
    __host__ __device__ int levels() const { return 1 << depth; }
    __device__ int component(const uint8_t* row, int i) const {
        if constexpr (Container == 0) return row[i];
        if constexpr (Container == 1) return ((int)((const uint16_t*)row)[i] >> lsb) & ((1 << depth) - 1);
        if constexpr (Container == 2) return (int)(((const uint32_t*)row)[i / 3] >> (10 * (i % 3))) & 1023;
    }
    __device__ int operator()(int64_t m, int c, int y, int x) const {
        const bool r = m >= N;
        const uint8_t* row = (r ? right.data : left.data) + (r ? m - N : m) * (r ? right.frame_stride : left.frame_stride) + (int64_t)y * (r ? right.pitch : left.pitch);
        const int p = x + (r ? right.x0 : left.x0), pair = (p >> 1) * 4, a = order & 1;
        // the three channels of a pixel repeat these loads; they are the same addresses, and the compiler merges them
        const int mid = 1 << (depth - 1), top = (1 << depth) - 1;          // from here on: yuv_source's conversion, statement for statement
        const int d = component(row, 2 * p + a) - mat.y_off, e = component(row, pair + 1 - a + (order & 2)) - mid, f = component(row, pair + 3 - order) - mid;
        const int acc = mat.cy * d + (c == 0 ? mat.crv * f : c == 1 ? -mat.cgu * e - mat.cgv * f : mat.cbu * e) + (1 << (mat.shift - 1));
        const int q = acc >> mat.shift;                                   // arithmetic shift: floor
        return q < 0 ? 0 : (q > top ? top : q);
    }
};

// interleaved RGB (ppms_video_ingest_rgb_packed): one pitched surface per view whose rows are streams of pixels, `step` components each (3, or 4 with
// a fourth that is never loaded: alpha travels nowhere).  Column x of the view is surface column p = x + x0 (any x0 >= 0: there is no chroma pair to
// split), and channel c is component step p + offset[c] of the row: container 0 byte i, 1 little-endian 16-bit word i, (word >> lsb) masked to `depth`
// bits, as yuv_packed_source::component reads them; container 2 (step 1) field offset[c] -- bits [10 f, 10 f + 10) -- of 32-bit word p, bits 30 and 31
// ignored.  Loads are of one container element (the host checks the alignment of pointers and strides for 16- and 32-bit elements); every offset is
// 64-bit.  (y, x) arrives clamped into the hs x ws frame, so p <= P - 1 with P = x0 + ws, and with offset[c] <= step - 1 the largest component index is
// step P - 1 (container 2: word P - 1): inside the step P bytes, 2 step P bytes or 4 P bytes the host demands of the pitch.  No load leaves
// [row, row + row_bytes).  The sample is the level: no conversion follows.
template <int Container>
struct rgb_packed_source {
    ppms_packed_view left, right;
    int N, depth, lsb, step, offset_r, offset_g, offset_b;                // uniform: the ppms_rgb_packed_format
    static constexpr bool table_by_depth = true;
    __host__ __device__ int levels() const { return 1 << depth; }
    __device__ int operator()(int64_t m, int c, int y, int x) const {
        const bool r = m >= N;
        const uint8_t* row = (r ? right.data : left.data) + (r ? m - N : m) * (r ? right.frame_stride : left.frame_stride) + (int64_t)y * (r ? right.pitch : left.pitch);
        const int64_t p = x + (r ? right.x0 : left.x0);
        const int o = c == 0 ? offset_r : c == 1 ? offset_g : offset_b;
        if constexpr (Container == 0) return row[step * p + o];
        if constexpr (Container == 1) return ((int)((const uint16_t*)row)[step * p + o] >> lsb) & ((1 << depth) - 1);
        if constexpr (Container == 2) return (int)(((const uint32_t*)row)[p] >> (10 * o)) & 1023;
    }
};

// channel c of pixel (y, x) of a raw source `f` (its hs, ws, depth, pattern, black, gains and shift) whose sample at a frame coordinate is s(yy, xx):
// the demosaic, black level and white balance of the raw sources, unpacked and packed.  With (y, x) inside the hs x ws frame and hs, ws >= 2 (the
// host refuses less for a colour pattern) every coordinate handed to s lies inside the frame.
template <class Source, class Sample>
__device__ __forceinline__ int raw_level(const Source& f, int c, int y, int x, Sample s) {
    const int hs = f.hs, ws = f.ws, pattern = f.pattern;
    int v;
    if (pattern == 4) {                                                   // MONO
        v = s(y, x);
    } else {
        const int ym = y > 0 ? y - 1 : 1, yp = y < hs - 1 ? y + 1 : hs - 2, xm = x > 0 ? x - 1 : 1, xp = x < ws - 1 ? x + 1 : ws - 2;
        const bool green = ((x ^ y ^ (pattern >> 1)) & 1) != 0, red_row = ((y ^ pattern) & 1) == 0;
        if (c == (green ? 1 : (red_row ? 0 : 2)))
            v = s(y, x);
        else if (green)                                                   // R or B at a green site: the two neighbours that carry it
            v = (c == 0) == red_row ? (s(y, xm) + s(y, xp) + 1) >> 1 : (s(ym, x) + s(yp, x) + 1) >> 1;
        else if (c == 1)                                                  // G at a red or blue site
            v = (s(ym, x) + s(yp, x) + s(y, xm) + s(y, xp) + 2) >> 2;
        else                                                              // B at a red site, R at a blue site
            v = (s(ym, xm) + s(ym, xp) + s(yp, xm) + s(yp, xp) + 2) >> 2;
    }
    const int top = (1 << f.depth) - 1;
    const int q = ((v - f.black) * (c == 0 ? f.gain_r : c == 1 ? f.gain_g : f.gain_b) + (1 << (f.shift - 1))) >> f.shift;     // arithmetic shift: floor
    return q < 0 ? 0 : (q > top ? top : q);
}

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
        return raw_level(*this, c, y, x, [&](int yy, int xx) { return ((int)*(const T*)(p + yy * pitch + (int64_t)xx * (int)sizeof(T)) >> lsb) & top; });
    }
};

// the same frames in a packed transport format (ppms_video_ingest_raw_packed): 10- or 12-bit samples without padding bits, one pitched surface per
// view.  Column xx of the view is surface column q = xx + x0 (any x0 >= 0: the pattern is that of the view's own pixel (0, 0)).
//   Packing 0 (MIPI CSI-2): RAW10 keeps the top 8 bits of pixels 4 g .. 4 g + 3 in bytes 5 g .. 5 g + 3 and their low 2 bits in byte 5 g + 4, pixel
// k's at bits [2 k, 2 k + 2); RAW12 the top 8 bits of pixels 2 g, 2 g + 1 in bytes 3 g, 3 g + 1 and their low 4 bits in the nibbles of byte 3 g + 2.
//   Packing 1 (PFNC 10p / 12p): an lsb-first bit stream, pixel q at bits [q depth, q depth + depth): with depth in {10, 12} that is (bit & 7) in
// {0, 2, 4, 6} or {0, 4}, so the pixel lies in exactly the two bytes o, o + 1 of o = bit >> 3, and both hold bits of the pixel itself.
// Byte loads only.  raw_level hands over coordinates inside the hs x ws frame, so q <= P - 1 with P = x0 + ws: the last byte read is that of the
// last group, 5 ceil(P / 4) - 1 or 3 ceil(P / 2) - 1, or the last byte of pixel P - 1, ceil(P depth / 8) - 1 -- inside the row_bytes the host demands
// of the pitch.  No load leaves [row, row + row_bytes).
template <int Packing>
struct raw_packed_source {
    ppms_packed_view left, right;
    int N, hs, ws;                                                        // frames per view, the SOURCE frame size
    int depth, pattern, black, gain_r, gain_g, gain_b, shift;             // uniform: the ppms_raw_packed_format
    static constexpr bool table_by_depth = true;
    __host__ __device__ int levels() const { return 1 << depth; }
    __device__ int operator()(int64_t m, int c, int y, int x) const {
        const bool r = m >= N;
        const uint8_t* p = (r ? right.data : left.data) + (r ? m - N : m) * (r ? right.frame_stride : left.frame_stride);
        const int64_t pitch = r ? right.pitch : left.pitch;
        const int x0 = r ? right.x0 : left.x0;
        // the three channels of a pixel repeat these loads; they are the same addresses, and the compiler merges them
        return raw_level(*this, c, y, x, [&](int yy, int xx) {
            const uint8_t* row = p + yy * pitch;
            const int q = xx + x0;
            if constexpr (Packing == 0) {
                if (depth == 10) {
                    const int g = (q >> 2) * 5, k = q & 3;
                    return (int)row[g + k] << 2 | (((int)row[g + 4] >> (2 * k)) & 3);
                }
                const int g = (q >> 1) * 3, k = q & 1;
                return (int)row[g + k] << 4 | (((int)row[g + 2] >> (4 * k)) & 15);
            } else {
                const int bit = q * depth, o = bit >> 3;
                return (((int)row[o] | (int)row[o + 1] << 8) >> (bit & 7)) & ((1 << depth) - 1);
            }
        });
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

// colour out (ppms_video_colour_*): the left view behind the same Source as 4-byte pixels registered to the egress planes.  Thread = a run of
// COLOUR_RUN consecutive x of one output row: output pixel (f, y, x) is source pixel (clamp(y + y0), clamp(x + x0)) of image frame0 + f < N (the
// left view: a Source's right half is never reached), its three levels go through `table` -- uint8, 256 or source.levels() entries, the byte each
// level stands for, the caller's arithmetic -- held in LDS as the ingest kernel holds its float table, and the pixel is R | G << 8 | B << 16 |
// 255 << 24 (`bgr`: B and R swapped).  A whole run at a 16-byte aligned address is one 16-byte store, anything else 4-byte stores; every offset is
// 64-bit; bytes between the rows of a pitched plane are not written.
constexpr int COLOUR_RUN = 4;
template <class Source>
__global__ __launch_bounds__(256) void video_colour_kernel(Source source, int H0, int W0, int frame0, int x0, int y0, int h0, int w0, int bgr,
                                                           const uint8_t* __restrict__ table, ppms_egress_plane out, int rpr, int64_t total) {
    const uint8_t* tab;
    if constexpr (Source::table_by_depth) {                               // 1 << depth bytes of dynamic LDS (sized by the launch)
        extern __shared__ uint8_t level_bytes[];
        for (int i = threadIdx.x, n = source.levels(); i < n; i += 256) level_bytes[i] = table[i];
        tab = level_bytes;
    } else {
        __shared__ uint8_t byte_bytes[256];
        byte_bytes[threadIdx.x] = table[threadIdx.x];
        tab = byte_bytes;
    }
    __syncthreads();
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int xs = (int)(idx % rpr) * COLOUR_RUN;
    const int64_t row = idx / rpr;                                       // f * h0 + y of the output
    const int y = (int)(row % h0);
    const int64_t f = row / h0;
    const int n = w0 - xs < COLOUR_RUN ? w0 - xs : COLOUR_RUN;           // pixels of this run inside the row
    const int64_t yy = (int64_t)y + y0;
    const int sy = yy < 0 ? 0 : (yy > H0 - 1 ? H0 - 1 : (int)yy);       // replicate padding, as the ingest kernel clamps
    uint32_t px[COLOUR_RUN];
#pragma unroll
    for (int j = 0; j < COLOUR_RUN; ++j) {
        const int64_t xx = (int64_t)xs + (j < n ? j : n - 1) + x0;       // (past the row's end the last pixel again: never stored)
        const int sx = xx < 0 ? 0 : (xx > W0 - 1 ? W0 - 1 : (int)xx);
        const uint32_t r = tab[source(frame0 + f, 0, sy, sx)], g = tab[source(frame0 + f, 1, sy, sx)], b = tab[source(frame0 + f, 2, sy, sx)];
        px[j] = (bgr ? b | r << 16 : r | b << 16) | g << 8 | 0xff000000u;
    }
    uint32_t* dst = (uint32_t*)((char*)out.ptr + f * out.frame_stride + (int64_t)y * out.pitch) + xs;
    if (n == COLOUR_RUN && ((uintptr_t)dst & 15) == 0) {
        gstore16(dst, __builtin_bit_cast(u32x4, px));
    } else {
#pragma unroll
        for (int j = 0; j < COLOUR_RUN; ++j)
            if (j < n) gst<uint32_t>(dst + j, px[j]);
    }
}

}  // namespace

// ---- host side: every entry point fills one ingest_call, runs its door's checks and goes through ingest_samples() to the one launch ----------

// what all 14 entry points take behind their source: the entry's name for the messages, geometry, table, destinations and stream
struct colour_call;
struct ingest_call {
    const char* who;
    int N, H0, W0, pad_left, pad_top, H, W;
    const float* lut;
    ppms_sp dst_fnet, dst_cnet;
    void* stream;
    const colour_call* colour = nullptr;                                  // a ppms_video_colour_* call: the launch behind the door's checks is the colour kernel's
};
// what the 14 colour entry points take behind N, H0, W0 (`lut` of their ingest_call is `table`, for the doors' null checks only)
struct colour_call {
    int frame0, n_frames, x0, y0, h0, w0;
    const uint8_t* table;
    const ppms_egress_plane* out;
};

// what every entry point checks about sizes, pads, table and destinations, and its launch
template <class Source>
static int video_ingest_launch(const ingest_call& a, const Source& source) {
    const char* who = a.who;
    const int N = a.N, H0 = a.H0, W0 = a.W0, pad_left = a.pad_left, pad_top = a.pad_top, H = a.H, W = a.W;
    PPMS_REQUIRE(a.lut, "%s: null table pointer", who);
    PPMS_REQUIRE(N > 0 && H0 > 0 && W0 > 0 && H > 0 && W > 0, "%s: N = %d, H0 = %d, W0 = %d, H = %d, W = %d must be positive", who, N, H0, W0, H, W);
    PPMS_REQUIRE(H % 4 == 0 && W % 4 == 0, "%s: H = %d, W = %d must be multiples of 4", who, H, W);
    PPMS_REQUIRE(pad_left >= 0 && pad_top >= 0 && (int64_t)pad_top + H0 <= H && (int64_t)pad_left + W0 <= W,
                 "%s: pad_left = %d, pad_top = %d with a %d x %d source do not fit the %d x %d padded image", who, pad_left, pad_top, H0, W0, H, W);
    PPMS_REQUIRE(a.dst_fnet.hi || a.dst_cnet.hi, "%s: both destinations skipped", who);
    const ppms_sp* dsts[2] = {&a.dst_fnet, &a.dst_cnet};
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
    hipLaunchKernelGGL(video_ingest_kernel<Source>, dim3(ceil_div(total, 256)), dim3(256), table_bytes, (hipStream_t)a.stream, source, N, H0, W0, pad_left, pad_top,
                       H, W, a.lut, a.dst_fnet, a.dst_cnet, threads[0], total);
    return ppms_check_launch(who);
}

// what every colour entry point checks behind its door -- the table, sizes, the plane, the frame range and the rectangle -- and its launch
template <class Source>
static int video_colour_launch(const ingest_call& a, const Source& source) {
    const char* who = a.who;
    const colour_call& c = *a.colour;
    PPMS_REQUIRE(c.table, "%s: null table pointer", who);
    PPMS_REQUIRE(a.N > 0 && a.H0 > 0 && a.W0 > 0, "%s: N = %d, H0 = %d, W0 = %d must be positive", who, a.N, a.H0, a.W0);
    PPMS_REQUIRE(c.n_frames > 0, "%s: n_frames = %d must be positive", who, c.n_frames);
    PPMS_REQUIRE(c.frame0 >= 0 && (int64_t)c.frame0 + c.n_frames <= a.N, "%s: frame0 = %d, n_frames = %d leave the N = %d frames", who, c.frame0, c.n_frames, a.N);
    PPMS_REQUIRE(c.h0 > 0 && c.w0 > 0, "%s: h0 = %d, w0 = %d must be positive", who, c.h0, c.w0);
    if (const int rc = egress_check_colour_plane(who, "out", c.out, c.n_frames, c.h0, c.w0)) return rc;
    const int rpr = (c.w0 + COLOUR_RUN - 1) / COLOUR_RUN;                 // runs per output row
    const int64_t total = (int64_t)c.n_frames * c.h0 * rpr;
    PPMS_REQUIRE((total + 255) / 256 <= 0x7fffffff, "%s: %lld threads exceed one grid", who, (long long)total);
    size_t table_bytes = 0;                                                // dynamic LDS: the byte table of a source that sizes it by depth
    if constexpr (Source::table_by_depth) table_bytes = (size_t)source.levels();
    hipLaunchKernelGGL(video_colour_kernel<Source>, dim3(ceil_div(total, 256)), dim3(256), table_bytes, (hipStream_t)a.stream, source, a.H0, a.W0, c.frame0, c.x0,
                       c.y0, c.h0, c.w0, c.out->format == PPMS_FMT_BGRA8 ? 1 : 0, c.table, *c.out, rpr, total);
    return ppms_check_launch(who);
}

// what the remap entry points check about the two maps of a W0 columns wide rectified frame (`fill_max`: the top level of the source's samples)
static int remap_check(const char* who, const ppms_remap_view* lmap, const ppms_remap_view* rmap, int W0, int fill_max) {
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

// how a door's samples are stored: the head that ppms_yuv_format and ppms_raw_format share
struct sample_format {
    int sample_bytes, depth, lsb;
};
template <class Format>
static int depth_of(const Format* f) {                                    // (a null format reads as bytes here and is refused by the door's own check)
    return f ? f->depth : 8;
}
template <class Format>
static sample_format sample_format_of(const Format* f) {
    return f ? sample_format{f->sample_bytes, f->depth, f->lsb} : sample_format{1, 8, 0};
}

// how every format door's check opens: the pointers it needs (`pointers`: what the door's message calls them) and frames of a positive size, named
// `hname` x `wname` in the messages
static int opening_check(const ingest_call& a, bool all_there, const char* pointers, int H0, int W0, const char* hname, const char* wname) {
    PPMS_REQUIRE(all_there, "%s: null %s pointer", a.who, pointers);
    PPMS_REQUIRE(a.N > 0 && H0 > 0 && W0 > 0, "%s: N = %d, %s = %d, %s = %d must be positive", a.who, a.N, hname, H0, wname, W0);
    return PPMS_OK;
}

static int sample_format_check(const char* who, const sample_format& f) {
    const int sb = f.sample_bytes;
    PPMS_REQUIRE(sb == 1 || sb == 2, "%s: sample_bytes = %d must be 1 or 2", who, sb);
    PPMS_REQUIRE(sb == 1 ? f.depth == 8 : (f.depth == 10 || f.depth == 12),
                 "%s: depth = %d does not go with sample_bytes = %d (8 with 1; 10 or 12 with 2)", who, f.depth, sb);
    PPMS_REQUIRE(f.lsb == 0 || (sb == 2 && f.lsb == 16 - f.depth), "%s: lsb = %d must be 0, or 16 - depth for 16-bit words", who, f.lsb);
    return PPMS_OK;
}

// one pitched plane of a view's frames -- `rows` rows of `row_bytes` (a row's first sample to the end of its last) -- and how the messages name it
struct plane_extent {
    const char *suffix, *kind, *whole;                                    // "_y", "luma ", "luma plane" / "_c", "chroma ", "chroma plane" / "", "", "frame"
    int64_t frame_stride;
    int pitch, rows;
    int64_t row_bytes;
    const char* wname;                                                    // the row's width in samples, named in the pitch message (nullptr: left out)
    int width;
};

// the planes of one view (`pointers`: all their base pointers or-ed together): even pointers and strides under 16-bit samples, every pitch >= its
// row, every frame stride >= its plane -- in that order over all planes.  `any_stride_of_one_frame`: the raw door never adds a single frame's stride
static int plane_extent_check(const char* who, const char* side, int sample_bytes, uintptr_t pointers, const plane_extent* planes, int count,
                              bool any_stride_of_one_frame) {
    if (sample_bytes == 2) {
        uintptr_t bits = pointers;
        for (int i = 0; i < count; ++i) bits |= (uintptr_t)planes[i].frame_stride | (uintptr_t)planes[i].pitch;
        PPMS_REQUIRE((bits & 1) == 0, "%s: %s view: an odd pointer or stride; 16-bit samples need even pointers, pitches and frame strides", who, side);
    }
    for (int i = 0; i < count; ++i) {
        const plane_extent& p = planes[i];
        char width[48] = "";
        if (p.wname) snprintf(width, sizeof(width), " (%s = %d)", p.wname, p.width);
        PPMS_REQUIRE(p.pitch >= p.row_bytes, "%s: %s pitch%s = %d is less than a %srow's %lld bytes%s", who, side, p.suffix, p.pitch, p.kind, (long long)p.row_bytes,
                     width);
    }
    for (int i = 0; i < count; ++i) {
        const plane_extent& p = planes[i];
        PPMS_REQUIRE(any_stride_of_one_frame || p.frame_stride >= (int64_t)(p.rows - 1) * p.pitch + p.row_bytes, "%s: %s frame_stride%s = %lld is less than a %s",
                     who, side, p.suffix, (long long)p.frame_stride, p.whole);
    }
    return PPMS_OK;
}

// the matrix of all six YUV entry points at samples of `depth` bits.  `shift_max`: the 4:2:0 entries accept shift up to 20, every other one up to
// 26 - depth (18 at depth 8); both keep every sum inside 32 bits
static int yuv_matrix_check(const char* who, const ppms_yuv_matrix* m, int depth, int shift_max) {
    PPMS_REQUIRE(m->shift >= 8 && m->shift <= shift_max, "%s: shift = %d must lie in [8, %d] at depth %d", who, m->shift, shift_max, depth);
    PPMS_REQUIRE(m->reserved == 0, "%s: matrix: reserved = %d must be 0", who, m->reserved);
    // coefficients below 4.0 keep every sum of the conversion inside 32 bits: three terms below 4 * 2^shift * 2^depth <= 2^28 each, plus 2^(shift - 1)
    // (the 4:2:0 entries' shift = 20: 2^22 (255 + 128 + 128) + 2^19 < 2^31)
    const int32_t lim = 4 << m->shift;
    PPMS_REQUIRE(m->y_off >= 0 && m->y_off < (1 << depth) && m->cy >= 0 && m->cy < lim && m->crv >= 0 && m->crv < lim && m->cgu >= 0 && m->cgu < lim &&
                     m->cgv >= 0 && m->cgv < lim && m->cbu >= 0 && m->cbu < lim,
                 "%s: y_off must lie in [0, %d] and every coefficient in [0, 4 << shift)", who, (1 << depth) - 1);
    return PPMS_OK;
}

// what ppms_raw_format and ppms_raw_packed_format share (their `depth` is checked before): pattern, black level, shift and gains, the format's
// reserved words (3 and 4 of them), and the 2 x 2 rule of a colour pattern for frames of H0 x W0 -- in that order
template <class Format>
static int raw_format_check(const char* who, const Format& f, int H0, int W0, const char* hname, const char* wname) {
    PPMS_REQUIRE(f.pattern >= 0 && f.pattern <= 4, "%s: pattern = %d must be 0 (RGGB), 1 (BGGR), 2 (GRBG), 3 (GBRG) or 4 (MONO)", who, f.pattern);
    PPMS_REQUIRE(f.black >= 0 && f.black < (1 << f.depth), "%s: black = %d must lie in [0, %d]", who, f.black, (1 << f.depth) - 1);
    PPMS_REQUIRE(f.shift >= 4 && f.shift <= 14, "%s: shift = %d must lie in [4, 14]", who, f.shift);
    // gains below 16.0 keep every sum inside 32 bits: 2^12 * 2^18 + 2^13 < 2^31 at depth 12 and shift = 14
    const int32_t lim = 16 << f.shift;
    PPMS_REQUIRE(f.gain[0] >= 0 && f.gain[0] < lim && f.gain[1] >= 0 && f.gain[1] < lim && f.gain[2] >= 0 && f.gain[2] < lim,
                 "%s: every gain must lie in [0, 16 << shift)", who);
    int32_t reserved = 0;
    for (const int32_t r : f.reserved) reserved |= r;
    PPMS_REQUIRE(reserved == 0, "%s: format: reserved must be 0", who);
    PPMS_REQUIRE(f.pattern == 4 || (H0 >= 2 && W0 >= 2), "%s: a colour pattern needs a frame of at least 2 x 2, got %s = %d, %s = %d", who, hname, H0, wname, W0);
    return PPMS_OK;
}

// what the four YUV entry points check about the format, the views (frames of H0 x W0, named `hname` x `wname` in the messages) and the matrix.
// (`shift_max`: yuv_matrix_check's)
static int yuv_check(const ingest_call& a, const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, const ppms_yuv_format* fmt,
                     int shift_max, int H0, int W0, const char* hname, const char* wname) {
    const char* who = a.who;
    if (const int rc = opening_check(a, left && right && m && fmt && a.lut, "view, matrix, format or table", H0, W0, hname, wname)) return rc;
    const ppms_yuv_format& f = *fmt;
    const int sb = f.sample_bytes;
    if (const int rc = sample_format_check(who, sample_format_of(fmt))) return rc;
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
        const plane_extent planes[2] = {{"_y", "luma ", "luma plane", v.frame_stride_y, v.pitch_y, H0, (int64_t)W0 * sb, wname, W0},
                                        {"_c", "chroma ", "chroma plane", v.frame_stride_c, v.pitch_c, Hc, (int64_t)v.step_c * (Wc - 1) + sb, nullptr, 0}};
        if (const int rc = plane_extent_check(who, side, sb, (uintptr_t)v.y | (uintptr_t)v.u | (uintptr_t)v.v, planes, 2, false)) return rc;
    }
    return yuv_matrix_check(who, m, f.depth, shift_max);
}

// what both ppms_video_ingest_raw entry points check about the format and the views (frames of H0 x W0, named `hname` x `wname` in the messages)
static int raw_check(const ingest_call& a, const ppms_raw_view* left, const ppms_raw_view* right, const ppms_raw_format* fmt, int H0, int W0,
                     const char* hname, const char* wname) {
    const char* who = a.who;
    if (const int rc = opening_check(a, left && right && fmt && a.lut, "view, format or table", H0, W0, hname, wname)) return rc;
    const ppms_raw_format& f = *fmt;
    if (const int rc = sample_format_check(who, sample_format_of(fmt))) return rc;
    if (const int rc = raw_format_check(who, f, H0, W0, hname, wname)) return rc;
    const ppms_raw_view* views[2] = {left, right};
    for (int s = 0; s < 2; ++s) {
        const ppms_raw_view& v = *views[s];
        const char* side = s == 0 ? "left" : "right";
        PPMS_REQUIRE(v.data, "%s: null data pointer in the %s view", who, side);
        PPMS_REQUIRE(v.reserved == 0, "%s: %s view: reserved = %d must be 0", who, side, v.reserved);
        const plane_extent plane{"", "", "frame", v.frame_stride, v.pitch, H0, (int64_t)W0 * f.sample_bytes, wname, W0};
        if (const int rc = plane_extent_check(who, side, f.sample_bytes, (uintptr_t)v.data, &plane, 1, a.N == 1)) return rc;
    }
    return PPMS_OK;
}

// the rectification maps of a _remap entry point (a plain entry point passes none: nullptr)
struct remap_maps {
    const ppms_remap_view *left, *right;
};

// the way of all 14 entry points: the maps' check (with them the source frames are the maps' hs x ws, not H0 x W0), the door's own `check(hs, ws,
// hname, wname)` of its views against those frames, then `pick(launch, hs, ws)`, which hands the door's source for frames of hs x ws to `launch` --
// the one launch, behind the maps if there are any.  `fill` of a map is a level of the format's `depth` (a format that names no depth is refused
// by `check`, right behind the maps, which bound hs and ws for it)
template <class Check, class Pick>
static int ingest_frames(const ingest_call& a, int depth, const remap_maps* maps, Check check, Pick pick) {
    int hs = a.H0, ws = a.W0;
    if (maps) {
        if (const int rc = remap_check(a.who, maps->left, maps->right, a.W0, depth == 10 || depth == 12 ? (1 << depth) - 1 : 255)) return rc;
        hs = maps->left->hs, ws = maps->left->ws;
    }
    if (const int rc = check(hs, ws, maps ? "hs" : "H0", maps ? "ws" : "W0")) return rc;
    const auto behind = [&](const auto& source) { return a.colour ? video_colour_launch(a, source) : video_ingest_launch(a, source); };
    const auto launch = [&](auto inner) {
        if (!maps) return behind(inner);
        return behind(remapped_source<decltype(inner)>{inner, *maps->left, *maps->right, a.N});
    };
    return pick(launch, hs, ws);
}

// the unpacked doors: `make(T{}, hs, ws)` is the door's source reading samples of T
template <class Check, class Make>
static int ingest_samples(const ingest_call& a, const sample_format& f, const remap_maps* maps, Check check, Make make) {
    return ingest_frames(a, f.depth, maps, check,
                         [&](auto launch, int hs, int ws) { return f.sample_bytes == 1 ? launch(make(uint8_t{}, hs, ws)) : launch(make(uint16_t{}, hs, ws)); });
}

static int ingest_u8(const ingest_call& a, const uint8_t* left, const uint8_t* right, int64_t frame_stride, const remap_maps* maps) {
    PPMS_REQUIRE(left && right, "%s: null source pointer", a.who);
    return ingest_samples(
        a, sample_format{1, 8, 0}, maps,
        [&](int hs, int ws, const char* hname, const char* wname) -> int {
            PPMS_REQUIRE(frame_stride >= (int64_t)3 * hs * ws, "%s: frame_stride = %lld is less than a %sframe's 3 * %s * %s bytes", a.who, (long long)frame_stride,
                         maps ? "source " : "", hname, wname);
            return PPMS_OK;
        },
        [&](auto, int hs, int ws) { return rgb_planes_source{left, right, frame_stride, a.N, hs, ws}; });
}

template <class Make>
static int ingest_yuv(const ingest_call& a, const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, const ppms_yuv_format* fmt,
                      int shift_max, const remap_maps* maps, Make make) {
    return ingest_samples(
        a, sample_format_of(fmt), maps,
        [&](int hs, int ws, const char* hname, const char* wname) { return yuv_check(a, left, right, m, fmt, shift_max, hs, ws, hname, wname); }, make);
}

// the yuv420 entry points: checked as the format {1, 8, 0, 1, 1} with shift up to 20 (the generic entries stop at 26 - 8), read by yuv420_source --
// yuv_source<uint8_t> writes the same bits and takes a tenth longer (docs/LOG_r10.md)
static int ingest_yuv420(const ingest_call& a, const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, const remap_maps* maps) {
    static const ppms_yuv_format bytes_420 = {1, 8, 0, 1, 1, {0, 0, 0}};
    return ingest_yuv(a, left, right, m, &bytes_420, 20, maps, [&](auto, int, int) { return yuv420_source{*left, *right, *m, a.N}; });
}

static int ingest_yuv_format(const ingest_call& a, const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, const ppms_yuv_format* f,
                             const remap_maps* maps) {
    return ingest_yuv(a, left, right, m, f, 26 - depth_of(f), maps,
                      [&](auto sample, int, int) { return yuv_source<decltype(sample)>{*left, *right, *m, a.N, f->depth, f->lsb, f->sub_x, f->sub_y}; });
}

static int ingest_raw(const ingest_call& a, const ppms_raw_view* left, const ppms_raw_view* right, const ppms_raw_format* f, const remap_maps* maps) {
    return ingest_samples(
        a, sample_format_of(f), maps,
        [&](int hs, int ws, const char* hname, const char* wname) { return raw_check(a, left, right, f, hs, ws, hname, wname); },
        [&](auto sample, int hs, int ws) {
            return raw_source<decltype(sample)>{*left, *right, a.N, hs, ws, f->depth, f->lsb, f->pattern, f->black, f->gain[0], f->gain[1], f->gain[2], f->shift};
        });
}

// what the six packed entry points check about one view's surface: x0 (even where `pair` says that a chroma pair may not be split), `align`-byte
// pointers and strides (`unit` names the container that needs them), a pitch that holds the row of P = x0 + W0 columns, and with N > 1 a frame
// stride that holds a frame.  `row_bytes(P)`: the format's row of P columns
template <class RowBytes>
static int packed_view_check(const ingest_call& a, const char* side, const ppms_packed_view& v, bool pair, int align, const char* unit, int H0, int W0,
                             const char* wname, RowBytes row_bytes) {
    const char* who = a.who;
    PPMS_REQUIRE(v.data, "%s: null data pointer in the %s view", who, side);
    PPMS_REQUIRE(v.x0 >= 0, "%s: %s x0 = %d must not be negative", who, side, v.x0);
    PPMS_REQUIRE(!pair || v.x0 % 2 == 0, "%s: %s x0 = %d must be even: a chroma pair may not be split", who, side, v.x0);
    PPMS_REQUIRE((int64_t)v.x0 + W0 <= 65536, "%s: %s x0 + %s = %d + %d exceeds 65536 columns", who, side, wname, v.x0, W0);
    PPMS_REQUIRE((((uintptr_t)v.data | (uintptr_t)v.frame_stride | (uintptr_t)v.pitch) & (uintptr_t)(align - 1)) == 0,
                 "%s: %s view: a misaligned pointer or stride; %s need pointers, pitches and frame strides that are multiples of %d", who, side, unit, align);
    const int64_t row = row_bytes(v.x0 + W0);
    PPMS_REQUIRE(v.pitch >= row, "%s: %s pitch = %d is less than a row's %lld bytes (x0 + %s = %d)", who, side, v.pitch, (long long)row, wname, v.x0 + W0);
    PPMS_REQUIRE(a.N == 1 || v.frame_stride >= (int64_t)(H0 - 1) * v.pitch + row, "%s: %s frame_stride = %lld is less than a frame", who, side,
                 (long long)v.frame_stride);
    return PPMS_OK;
}

// what both ppms_video_ingest_yuv_packed entry points check about the format, the views (frames of H0 x W0, named `hname` x `wname` in the messages)
// and the matrix (ppms_video_ingest_yuv's bounds: yuv_matrix_check)
static int yuv_packed_check(const ingest_call& a, const ppms_packed_view* left, const ppms_packed_view* right, const ppms_yuv_matrix* m,
                            const ppms_yuv_packed_format* fmt, int H0, int W0, const char* hname, const char* wname) {
    const char* who = a.who;
    if (const int rc = opening_check(a, left && right && m && fmt && a.lut, "view, matrix, format or table", H0, W0, hname, wname)) return rc;
    const ppms_yuv_packed_format& f = *fmt;
    PPMS_REQUIRE(f.container >= 0 && f.container <= 2, "%s: container = %d must be 0 (bytes), 1 (16-bit words) or 2 (v210)", who, f.container);
    PPMS_REQUIRE(f.order >= 0 && f.order <= 3, "%s: order = %d must be 0 (yuyv), 1 (uyvy), 2 (yvyu) or 3 (vyuy)", who, f.order);
    PPMS_REQUIRE(f.container == 0 ? f.depth == 8 : f.container == 1 ? (f.depth == 10 || f.depth == 12) : f.depth == 10,
                 "%s: depth = %d does not go with container = %d (8 with 0; 10 or 12 with 1; 10 with 2)", who, f.depth, f.container);
    PPMS_REQUIRE(f.container != 2 || f.order == 1, "%s: order = %d does not go with container = 2: v210 is uyvy (1)", who, f.order);
    PPMS_REQUIRE(f.lsb == 0 || (f.container == 1 && f.lsb == 16 - f.depth), "%s: lsb = %d must be 0, or 16 - depth for 16-bit words", who, f.lsb);
    PPMS_REQUIRE(f.reserved[0] == 0 && f.reserved[1] == 0 && f.reserved[2] == 0 && f.reserved[3] == 0, "%s: format: reserved must be 0", who);
    const int align = f.container == 0 ? 1 : f.container == 1 ? 2 : 4;
    const char* unit = f.container == 1 ? "16-bit words" : "v210's 32-bit words";
    const auto row_bytes = [&](int P) { return f.container == 2 ? (int64_t)16 * ((P + 5) / 6) : (int64_t)4 * align * ((P + 1) / 2); };
    if (const int rc = packed_view_check(a, "left", *left, true, align, unit, H0, W0, wname, row_bytes)) return rc;
    if (const int rc = packed_view_check(a, "right", *right, true, align, unit, H0, W0, wname, row_bytes)) return rc;
    return yuv_matrix_check(who, m, f.depth, 26 - f.depth);
}

// what both ppms_video_ingest_raw_packed entry points check about the format (ppms_video_ingest_raw's bounds: raw_format_check) and the views
static int raw_packed_check(const ingest_call& a, const ppms_packed_view* left, const ppms_packed_view* right, const ppms_raw_packed_format* fmt, int H0,
                            int W0, const char* hname, const char* wname) {
    const char* who = a.who;
    if (const int rc = opening_check(a, left && right && fmt && a.lut, "view, format or table", H0, W0, hname, wname)) return rc;
    const ppms_raw_packed_format& f = *fmt;
    PPMS_REQUIRE(f.packing == 0 || f.packing == 1, "%s: packing = %d must be 0 (MIPI CSI-2) or 1 (PFNC, lsb first)", who, f.packing);
    PPMS_REQUIRE(f.depth == 10 || f.depth == 12, "%s: depth = %d must be 10 or 12", who, f.depth);
    if (const int rc = raw_format_check(who, f, H0, W0, hname, wname)) return rc;
    const auto row_bytes = [&](int P) {
        return f.packing == 1 ? ((int64_t)P * f.depth + 7) / 8 : f.depth == 10 ? (int64_t)5 * ((P + 3) / 4) : (int64_t)3 * ((P + 1) / 2);
    };
    if (const int rc = packed_view_check(a, "left", *left, false, 1, "", H0, W0, wname, row_bytes)) return rc;
    return packed_view_check(a, "right", *right, false, 1, "", H0, W0, wname, row_bytes);
}

// what both ppms_video_ingest_rgb_packed entry points check about the format and the views (frames of H0 x W0, named `hname` x `wname` in the messages)
static int rgb_packed_check(const ingest_call& a, const ppms_packed_view* left, const ppms_packed_view* right, const ppms_rgb_packed_format* fmt, int H0,
                            int W0, const char* hname, const char* wname) {
    const char* who = a.who;
    if (const int rc = opening_check(a, left && right && fmt && a.lut, "view, format or table", H0, W0, hname, wname)) return rc;
    const ppms_rgb_packed_format& f = *fmt;
    PPMS_REQUIRE(f.container >= 0 && f.container <= 2, "%s: container = %d must be 0 (bytes), 1 (16-bit words) or 2 (one 32-bit word of three 10-bit fields)", who,
                 f.container);
    PPMS_REQUIRE(f.container == 0 ? f.depth == 8 : f.container == 1 ? (f.depth == 10 || f.depth == 12) : f.depth == 10,
                 "%s: depth = %d does not go with container = %d (8 with 0; 10 or 12 with 1; 10 with 2)", who, f.depth, f.container);
    PPMS_REQUIRE(f.lsb == 0 || (f.container == 1 && f.lsb == 16 - f.depth), "%s: lsb = %d must be 0, or 16 - depth for 16-bit words", who, f.lsb);
    PPMS_REQUIRE(f.container == 2 ? f.step == 1 : (f.step == 3 || f.step == 4), "%s: step = %d does not go with container = %d (3 or 4 with 0 and 1; 1 with 2)", who,
                 f.step, f.container);
    const int places = f.container == 2 ? 3 : f.step;                    // where a channel may lie: a component of the pixel, or a field of the word
    for (const int32_t o : f.offset)
        PPMS_REQUIRE(o >= 0 && o < places, "%s: offset = (%d, %d, %d) must lie in [0, %d)", who, f.offset[0], f.offset[1], f.offset[2], places);
    PPMS_REQUIRE(f.offset[0] != f.offset[1] && f.offset[0] != f.offset[2] && f.offset[1] != f.offset[2], "%s: offset = (%d, %d, %d): two channels in one place", who,
                 f.offset[0], f.offset[1], f.offset[2]);
    PPMS_REQUIRE(f.reserved == 0, "%s: format: reserved = %d must be 0", who, f.reserved);
    const int align = f.container == 0 ? 1 : f.container == 1 ? 2 : 4;
    const char* unit = f.container == 1 ? "16-bit words" : "32-bit words";
    const auto row_bytes = [&](int P) { return (int64_t)align * f.step * P; };
    if (const int rc = packed_view_check(a, "left", *left, false, align, unit, H0, W0, wname, row_bytes)) return rc;
    return packed_view_check(a, "right", *right, false, align, unit, H0, W0, wname, row_bytes);
}

static int ingest_yuv_packed(const ingest_call& a, const ppms_packed_view* left, const ppms_packed_view* right, const ppms_yuv_matrix* m,
                             const ppms_yuv_packed_format* f, const remap_maps* maps) {
    return ingest_frames(
        a, depth_of(f), maps,
        [&](int hs, int ws, const char* hname, const char* wname) { return yuv_packed_check(a, left, right, m, f, hs, ws, hname, wname); },
        [&](auto launch, int, int) {
            const auto source = [&](auto container) { return yuv_packed_source<decltype(container)::value>{*left, *right, *m, a.N, f->depth, f->lsb, f->order}; };
            if (f->container == 0) return launch(source(std::integral_constant<int, 0>{}));
            if (f->container == 1) return launch(source(std::integral_constant<int, 1>{}));
            return launch(source(std::integral_constant<int, 2>{}));
        });
}

static int ingest_raw_packed(const ingest_call& a, const ppms_packed_view* left, const ppms_packed_view* right, const ppms_raw_packed_format* f,
                             const remap_maps* maps) {
    return ingest_frames(
        a, depth_of(f), maps,
        [&](int hs, int ws, const char* hname, const char* wname) { return raw_packed_check(a, left, right, f, hs, ws, hname, wname); },
        [&](auto launch, int hs, int ws) {
            const auto source = [&](auto packing) {
                return raw_packed_source<decltype(packing)::value>{*left, *right, a.N, hs, ws, f->depth, f->pattern, f->black, f->gain[0], f->gain[1], f->gain[2], f->shift};
            };
            return f->packing == 0 ? launch(source(std::integral_constant<int, 0>{})) : launch(source(std::integral_constant<int, 1>{}));
        });
}

static int ingest_rgb_packed(const ingest_call& a, const ppms_packed_view* left, const ppms_packed_view* right, const ppms_rgb_packed_format* f,
                             const remap_maps* maps) {
    return ingest_frames(
        a, depth_of(f), maps,
        [&](int hs, int ws, const char* hname, const char* wname) { return rgb_packed_check(a, left, right, f, hs, ws, hname, wname); },
        [&](auto launch, int, int) {
            const auto source = [&](auto container) {
                return rgb_packed_source<decltype(container)::value>{*left, *right, a.N, f->depth, f->lsb, f->step, f->offset[0], f->offset[1], f->offset[2]};
            };
            if (f->container == 0) return launch(source(std::integral_constant<int, 0>{}));
            if (f->container == 1) return launch(source(std::integral_constant<int, 1>{}));
            return launch(source(std::integral_constant<int, 2>{}));
        });
}

// the trailing arguments every entry point declares, and the ingest_call they fill
#define INGEST_TAIL int N, int H0, int W0, int pad_left, int pad_top, int H, int W, const float* lut, ppms_sp dst_fnet, ppms_sp dst_cnet, void* stream
#define INGEST_CALL(name) ingest_call{name, N, H0, W0, pad_left, pad_top, H, W, lut, dst_fnet, dst_cnet, stream}

extern "C" int ppms_video_ingest_u8(const uint8_t* left, const uint8_t* right, int64_t frame_stride, INGEST_TAIL) {
    return ingest_u8(INGEST_CALL("video_ingest_u8"), left, right, frame_stride, nullptr);
}
extern "C" int ppms_video_ingest_u8_remap(const uint8_t* left, const uint8_t* right, int64_t frame_stride, const ppms_remap_view* lmap,
                                          const ppms_remap_view* rmap, INGEST_TAIL) {
    const remap_maps maps{lmap, rmap};
    return ingest_u8(INGEST_CALL("video_ingest_u8_remap"), left, right, frame_stride, &maps);
}

extern "C" int ppms_video_ingest_yuv420(const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, INGEST_TAIL) {
    return ingest_yuv420(INGEST_CALL("video_ingest_yuv420"), left, right, m, nullptr);
}
extern "C" int ppms_video_ingest_yuv420_remap(const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, const ppms_remap_view* lmap,
                                              const ppms_remap_view* rmap, INGEST_TAIL) {
    const remap_maps maps{lmap, rmap};
    return ingest_yuv420(INGEST_CALL("video_ingest_yuv420_remap"), left, right, m, &maps);
}

extern "C" int ppms_video_ingest_yuv(const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, const ppms_yuv_format* fmt, INGEST_TAIL) {
    return ingest_yuv_format(INGEST_CALL("video_ingest_yuv"), left, right, m, fmt, nullptr);
}
extern "C" int ppms_video_ingest_yuv_remap(const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, const ppms_yuv_format* fmt,
                                           const ppms_remap_view* lmap, const ppms_remap_view* rmap, INGEST_TAIL) {
    const remap_maps maps{lmap, rmap};
    return ingest_yuv_format(INGEST_CALL("video_ingest_yuv_remap"), left, right, m, fmt, &maps);
}

extern "C" int ppms_video_ingest_raw(const ppms_raw_view* left, const ppms_raw_view* right, const ppms_raw_format* fmt, INGEST_TAIL) {
    return ingest_raw(INGEST_CALL("video_ingest_raw"), left, right, fmt, nullptr);
}
extern "C" int ppms_video_ingest_raw_remap(const ppms_raw_view* left, const ppms_raw_view* right, const ppms_raw_format* fmt, const ppms_remap_view* lmap,
                                           const ppms_remap_view* rmap, INGEST_TAIL) {
    const remap_maps maps{lmap, rmap};
    return ingest_raw(INGEST_CALL("video_ingest_raw_remap"), left, right, fmt, &maps);
}

extern "C" int ppms_video_ingest_yuv_packed(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_yuv_matrix* m,
                                            const ppms_yuv_packed_format* fmt, INGEST_TAIL) {
    return ingest_yuv_packed(INGEST_CALL("video_ingest_yuv_packed"), left, right, m, fmt, nullptr);
}
extern "C" int ppms_video_ingest_yuv_packed_remap(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_yuv_matrix* m,
                                                  const ppms_yuv_packed_format* fmt, const ppms_remap_view* lmap, const ppms_remap_view* rmap, INGEST_TAIL) {
    const remap_maps maps{lmap, rmap};
    return ingest_yuv_packed(INGEST_CALL("video_ingest_yuv_packed_remap"), left, right, m, fmt, &maps);
}

extern "C" int ppms_video_ingest_raw_packed(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_raw_packed_format* fmt, INGEST_TAIL) {
    return ingest_raw_packed(INGEST_CALL("video_ingest_raw_packed"), left, right, fmt, nullptr);
}
extern "C" int ppms_video_ingest_raw_packed_remap(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_raw_packed_format* fmt,
                                                  const ppms_remap_view* lmap, const ppms_remap_view* rmap, INGEST_TAIL) {
    const remap_maps maps{lmap, rmap};
    return ingest_raw_packed(INGEST_CALL("video_ingest_raw_packed_remap"), left, right, fmt, &maps);
}

extern "C" int ppms_video_ingest_rgb_packed(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_rgb_packed_format* fmt, INGEST_TAIL) {
    return ingest_rgb_packed(INGEST_CALL("video_ingest_rgb_packed"), left, right, fmt, nullptr);
}
extern "C" int ppms_video_ingest_rgb_packed_remap(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_rgb_packed_format* fmt,
                                                  const ppms_remap_view* lmap, const ppms_remap_view* rmap, INGEST_TAIL) {
    const remap_maps maps{lmap, rmap};
    return ingest_rgb_packed(INGEST_CALL("video_ingest_rgb_packed_remap"), left, right, fmt, &maps);
}

// ---- colour out: the same 14 doors in front of video_colour_kernel.  The trailing arguments every colour entry point declares, and the ingest_call
// (its door's checks read who, N, H0, W0 and the table's null check) with the colour_call they fill
#define COLOUR_TAIL int N, int H0, int W0, int frame0, int n_frames, int x0, int y0, int h0, int w0, const uint8_t* table, const ppms_egress_plane* out, void* stream
#define COLOUR_CALL(name)                                                      \
    const colour_call colour{frame0, n_frames, x0, y0, h0, w0, table, out};    \
    const ingest_call call{name, N, H0, W0, 0, 0, 0, 0, (const float*)table, ppms_sp{}, ppms_sp{}, stream, &colour}

extern "C" int ppms_video_colour_u8(const uint8_t* left, const uint8_t* right, int64_t frame_stride, COLOUR_TAIL) {
    COLOUR_CALL("video_colour_u8");
    return ingest_u8(call, left, right, frame_stride, nullptr);
}
extern "C" int ppms_video_colour_u8_remap(const uint8_t* left, const uint8_t* right, int64_t frame_stride, const ppms_remap_view* lmap,
                                          const ppms_remap_view* rmap, COLOUR_TAIL) {
    COLOUR_CALL("video_colour_u8_remap");
    const remap_maps maps{lmap, rmap};
    return ingest_u8(call, left, right, frame_stride, &maps);
}
extern "C" int ppms_video_colour_yuv420(const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, COLOUR_TAIL) {
    COLOUR_CALL("video_colour_yuv420");
    return ingest_yuv420(call, left, right, m, nullptr);
}
extern "C" int ppms_video_colour_yuv420_remap(const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, const ppms_remap_view* lmap,
                                              const ppms_remap_view* rmap, COLOUR_TAIL) {
    COLOUR_CALL("video_colour_yuv420_remap");
    const remap_maps maps{lmap, rmap};
    return ingest_yuv420(call, left, right, m, &maps);
}
extern "C" int ppms_video_colour_yuv(const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, const ppms_yuv_format* fmt, COLOUR_TAIL) {
    COLOUR_CALL("video_colour_yuv");
    return ingest_yuv_format(call, left, right, m, fmt, nullptr);
}
extern "C" int ppms_video_colour_yuv_remap(const ppms_yuv_view* left, const ppms_yuv_view* right, const ppms_yuv_matrix* m, const ppms_yuv_format* fmt,
                                           const ppms_remap_view* lmap, const ppms_remap_view* rmap, COLOUR_TAIL) {
    COLOUR_CALL("video_colour_yuv_remap");
    const remap_maps maps{lmap, rmap};
    return ingest_yuv_format(call, left, right, m, fmt, &maps);
}
extern "C" int ppms_video_colour_raw(const ppms_raw_view* left, const ppms_raw_view* right, const ppms_raw_format* fmt, COLOUR_TAIL) {
    COLOUR_CALL("video_colour_raw");
    return ingest_raw(call, left, right, fmt, nullptr);
}
extern "C" int ppms_video_colour_raw_remap(const ppms_raw_view* left, const ppms_raw_view* right, const ppms_raw_format* fmt, const ppms_remap_view* lmap,
                                           const ppms_remap_view* rmap, COLOUR_TAIL) {
    COLOUR_CALL("video_colour_raw_remap");
    const remap_maps maps{lmap, rmap};
    return ingest_raw(call, left, right, fmt, &maps);
}
extern "C" int ppms_video_colour_yuv_packed(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_yuv_matrix* m,
                                            const ppms_yuv_packed_format* fmt, COLOUR_TAIL) {
    COLOUR_CALL("video_colour_yuv_packed");
    return ingest_yuv_packed(call, left, right, m, fmt, nullptr);
}
extern "C" int ppms_video_colour_yuv_packed_remap(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_yuv_matrix* m,
                                                  const ppms_yuv_packed_format* fmt, const ppms_remap_view* lmap, const ppms_remap_view* rmap, COLOUR_TAIL) {
    COLOUR_CALL("video_colour_yuv_packed_remap");
    const remap_maps maps{lmap, rmap};
    return ingest_yuv_packed(call, left, right, m, fmt, &maps);
}
extern "C" int ppms_video_colour_raw_packed(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_raw_packed_format* fmt, COLOUR_TAIL) {
    COLOUR_CALL("video_colour_raw_packed");
    return ingest_raw_packed(call, left, right, fmt, nullptr);
}
extern "C" int ppms_video_colour_raw_packed_remap(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_raw_packed_format* fmt,
                                                  const ppms_remap_view* lmap, const ppms_remap_view* rmap, COLOUR_TAIL) {
    COLOUR_CALL("video_colour_raw_packed_remap");
    const remap_maps maps{lmap, rmap};
    return ingest_raw_packed(call, left, right, fmt, &maps);
}

extern "C" int ppms_video_colour_rgb_packed(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_rgb_packed_format* fmt, COLOUR_TAIL) {
    COLOUR_CALL("video_colour_rgb_packed");
    return ingest_rgb_packed(call, left, right, fmt, nullptr);
}
extern "C" int ppms_video_colour_rgb_packed_remap(const ppms_packed_view* left, const ppms_packed_view* right, const ppms_rgb_packed_format* fmt,
                                                  const ppms_remap_view* lmap, const ppms_remap_view* rmap, COLOUR_TAIL) {
    COLOUR_CALL("video_colour_rgb_packed_remap");
    const remap_maps maps{lmap, rmap};
    return ingest_rgb_packed(call, left, right, fmt, &maps);
}

extern "C" int ppms_rgb_packed_struct_size(int* fmt) {
    if (fmt) *fmt = (int)sizeof(ppms_rgb_packed_format);
    return PPMS_OK;
}
extern "C" int ppms_packed_struct_sizes(int* view, int* yuv_format, int* raw_format) {
    if (view) *view = (int)sizeof(ppms_packed_view);
    if (yuv_format) *yuv_format = (int)sizeof(ppms_yuv_packed_format);
    if (raw_format) *raw_format = (int)sizeof(ppms_raw_packed_format);
    return PPMS_OK;
}
extern "C" int ppms_yuv_struct_sizes(int* view, int* matrix) {
    if (view) *view = (int)sizeof(ppms_yuv_view);
    if (matrix) *matrix = (int)sizeof(ppms_yuv_matrix);
    return PPMS_OK;
}
extern "C" int ppms_yuv_format_struct_size(int* fmt) {
    if (fmt) *fmt = (int)sizeof(ppms_yuv_format);
    return PPMS_OK;
}
extern "C" int ppms_remap_struct_size(int* view) {
    if (view) *view = (int)sizeof(ppms_remap_view);
    return PPMS_OK;
}
extern "C" int ppms_raw_struct_sizes(int* view, int* format) {
    if (view) *view = (int)sizeof(ppms_raw_view);
    if (format) *format = (int)sizeof(ppms_raw_format);
    return PPMS_OK;
}
