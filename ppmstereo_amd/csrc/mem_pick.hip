// Set-up of the memory read-out (ppmstereo_amd/engine.py): frame similarity, the QAM pick, the Q / K' operand kernels of the attention in
// mem_attn.hip, and the merged pick + key-modulation launch.
#include "common.h"

// ------------------------------------------------------------------------------------------------ frame similarity
// pooled[which][t][cell] = mean_c max_{adaptive window} x_t[c]  (AdaptiveMaxPool2d(h//4,w//4) + mean over channels)
__global__ __launch_bounds__(128) void qk_pool_kernel(const float* __restrict__ q, const float* __restrict__ k, int ld,
                                                      float* __restrict__ pooled, int T, int H, int W, int OH, int OW) {
    __shared__ float red[128];
    const int cell = blockIdx.x, t = blockIdx.y, which = blockIdx.z;
    const int oy = cell / OW, ox = cell - oy * OW;
    const int ys = (oy * H) / OH, ye = ((oy + 1) * H + OH - 1) / OH;
    const int xs = (ox * W) / OW, xe = ((ox + 1) * W + OW - 1) / OW;
    const float* src = (which ? k : q) + (int64_t)t * H * W * ld + threadIdx.x;
    float m = -INFINITY;
    for (int y = ys; y < ye; ++y)
        for (int x = xs; x < xe; ++x) m = fmaxf(m, src[((int64_t)y * W + x) * ld]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 64; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) pooled[((int64_t)which * T + t) * OH * OW + cell] = red[0] / 128.0f;
}
// sim[i][j] = cos(kbar_i, qbar_j), eps 1e-8 (F.cosine_similarity)
__global__ __launch_bounds__(64) void qk_cos_kernel(const float* __restrict__ pooled, float* __restrict__ sim, int T, int L) {
    const int i = blockIdx.y, j = blockIdx.x;
    const float* qv = pooled + (int64_t)j * L;
    const float* kv = pooled + ((int64_t)T + i) * L;
    float dot = 0.0f, nq = 0.0f, nk = 0.0f;
    for (int e = threadIdx.x; e < L; e += 64) {
        const float a = qv[e], b = kv[e];
        dot += a * b;
        nq += a * a;
        nk += b * b;
    }
    for (int s = 32; s > 0; s >>= 1) {
        dot += __shfl_xor(dot, s);
        nq += __shfl_xor(nq, s);
        nk += __shfl_xor(nk, s);
    }
    if (threadIdx.x == 0) sim[i * T + j] = dot / (fmaxf(sqrtf(nq), 1e-8f) * fmaxf(sqrtf(nk), 1e-8f));
}
// the two launches (arguments checked by the callers); the pool returns its number of cells
static int launch_qk_pool(const float* q, const float* k, int ld, float* pooled, int T, int H, int W, void* stream) {
    const int OH = H / 4, OW = W / 4;
    hipLaunchKernelGGL(qk_pool_kernel, dim3(OH * OW, T, 2), dim3(128), 0, (hipStream_t)stream, q, k, ld, pooled, T, H, W, OH, OW);
    return OH * OW;
}
static void launch_qk_cos(const float* pooled, float* sim, int T, int cells, void* stream) {
    hipLaunchKernelGGL(qk_cos_kernel, dim3(T, T), dim3(64), 0, (hipStream_t)stream, pooled, sim, T, cells);
}
extern "C" int ppms_qk_pool(const float* q, const float* k, int ld, float* pooled, int T, int H, int W, void* stream) {
    PPMS_REQUIRE(q && k && pooled && T > 0 && H >= 4 && W >= 4 && ld >= 128, "qk_pool: bad arguments (H,W >= 4)");
    launch_qk_pool(q, k, ld, pooled, T, H, W, stream);
    return ppms_check_launch("qk_pool");
}
extern "C" int ppms_qk_cos(const float* pooled, float* sim, int T, int cells, void* stream) {
    PPMS_REQUIRE(pooled && sim && T > 0 && cells > 0, "qk_cos: bad arguments");
    launch_qk_cos(pooled, sim, T, cells, stream);
    return ppms_check_launch("qk_cos");
}
extern "C" int ppms_qk_similarity(const float* q, const float* k, int ld, float* pooled, float* sim, int T, int H, int W, void* stream) {
    PPMS_REQUIRE(q && k && pooled && sim && T > 0 && H >= 4 && W >= 4 && ld >= 128, "qk_similarity: bad arguments (H,W >= 4)");
    launch_qk_cos(pooled, sim, T, launch_qk_pool(q, k, ld, pooled, T, H, W, stream), stream);
    return ppms_check_launch("qk_similarity");
}

// ------------------------------------------------------------------------------------------------ QAM pick
// one lane per clip row i: score[i][j] = exp(-S_ij / (sum_j S_ij + T)) * sim[i][j] + conf[j]; top-5 by score;
// S[i][sel] += 1; picked frames ascending + normalised scores s_hat = score / mean(score over picked)
//
// The pick as a workgroup-level function: every thread of the workgroup calls it (it holds a barrier), the lanes of ONE wave (`active`, lane
// index i) do the work; the picked-frame mask of clip i is returned to that lane (0 elsewhere).  conf: 64 floats of LDS; tab: 3 T T floats
// of LDS (usage counter | similarity | scores).  Everything the pick reads more than once is staged there by ONE round of global loads,
// issued by all threads together with the block sums of (up to) eight frames: read straight from global memory -- and the scores from a
// per-lane scratch array -- the pick was a chain of ~3 T dependent memory round trips, most of the 10 us a one-wave launch of it took.
// strive_out may be strive_in (in place: only picked entries are touched) or a second table, of which row i is then written whole (picked
// + 1, the rest copied); strive_out / sel / shat NULL = that result is not stored; sel / shat may point into LDS.
__device__ __forceinline__ unsigned long long qam_pick(const float* __restrict__ sim, const float* strive_in, float* strive_out,
                                                       const float* __restrict__ partial, int nblk, int HW, int32_t* sel, float* shat,
                                                       float* __restrict__ score_out, int T, float* conf, float* tab, bool active, int i) {
    const int TT = T * T;
    for (int e = threadIdx.x; e < TT; e += blockDim.x) {
        tab[e] = strive_in[e];
        tab[TT + e] = sim[e];
    }
    // frame confidences = mean of the uncertainty map: the block sums of frame f are added by all 64 lanes (lane l takes blocks l, l + 64,
    // ...; then a butterfly) -- a fixed order, the same on every rank of a sharded window.  Eight frames at a time, so that their loads are
    // in flight together (past the last frame the group repeats it and drops the result)
    if (active) {
        for (int f0 = 0; f0 < T; f0 += 8) {
            float s[8];
            const float* row[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                s[u] = 0.0f;
                row[u] = partial + (int64_t)(f0 + u < T ? f0 + u : T - 1) * nblk;
            }
            for (int b = i; b < nblk; b += 64)
#pragma unroll
                for (int u = 0; u < 8; ++u) s[u] += row[u][b];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) s[u] += __shfl_xor(s[u], m);
                if (i == 0 && f0 + u < T) conf[f0 + u] = s[u] / (float)HW;
            }
        }
    }
    __syncthreads();
    if (!active || i >= T) return 0ull;
    const float* st = tab + i * T;                       // this clip's rows: usage counter, similarity
    const float* sm = tab + TT + i * T;
    float* sc = tab + 2 * TT + i * T;                    // and its scores
    float ssum = 0.0f;
    for (int j = 0; j < T; ++j) ssum += st[j];
    const int ksel = T < 5 ? T : 5;
    unsigned long long picked = 0ull;
    for (int j = 0; j < T; ++j) {
        const float pen = expf(-st[j] / (ssum + (float)T));
        const float v = pen * sm[j] + conf[j];
        sc[j] = v;
        if (score_out) score_out[i * T + j] = v;
    }
    for (int n = 0; n < ksel; ++n) {
        int best = -1;
        float bv = -INFINITY;
        for (int j = 0; j < T; ++j) {
            if ((picked >> j) & 1ull) continue;
            const float v = sc[j];
            if (best < 0 || v > bv || (v != v && bv == bv)) {   // NaN scores (T == 1) still pick a frame
                best = j;
                bv = v;
            }
        }
        picked |= 1ull << best;
    }
    float mean = 0.0f;
    for (int j = 0; j < T; ++j)
        if ((picked >> j) & 1ull) mean += sc[j];
    mean /= (float)ksel;
    int n = 0;
    for (int j = 0; j < T; ++j) {
        const bool hit = (picked >> j) & 1ull;
        if (strive_out != nullptr) {
            if (hit)
                strive_out[i * T + j] = st[j] + 1.0f;
            else if (strive_out != strive_in)
                strive_out[i * T + j] = st[j];
        }
        if (hit) {
            if (sel != nullptr) {
                sel[i * 5 + n] = j;
                shat[i * 5 + n] = sc[j] / mean;
            }
            ++n;
        }
    }
    if (sel != nullptr)
        for (; n < 5; ++n) {
            sel[i * 5 + n] = 0;
            shat[i * 5 + n] = 0.0f;
        }
    return picked;
}
__global__ __launch_bounds__(64) void qam_select_kernel(const float* __restrict__ sim, float* strive, const float* __restrict__ partial, int nblk,
                                                        int HW, int32_t* __restrict__ sel, float* __restrict__ shat,
                                                        float* __restrict__ score_out, int T) {
    extern __shared__ __attribute__((aligned(16))) char qam_smem[];      // 3 T T floats
    __shared__ float conf[64];
    qam_pick(sim, strive, strive, partial, nblk, HW, sel, shat, score_out, T, conf, (float*)qam_smem, true, threadIdx.x);
}
extern "C" int ppms_qam_select(const float* sim, float* strive, const float* conf_partial, int nblk, int HW, int32_t* sel, float* shat,
                               float* score, int T, void* stream) {
    PPMS_REQUIRE(sim && strive && conf_partial && sel && shat && T > 0 && T <= 64, "qam_select: bad arguments (1 <= T <= 64)");
    hipLaunchKernelGGL(qam_select_kernel, dim3(1), dim3(64), (size_t)T * T * 12, (hipStream_t)stream, sim, strive, conf_partial, nblk, HW, sel, shat, score, T);
    return ppms_check_launch("qam_select");
}

// ------------------------------------------------------------------------------------------------ attention operands
__global__ __launch_bounds__(256) void attn_prep_q_kernel(const float* __restrict__ q, int ld, const float* __restrict__ pe,
                                                          bf16_t* __restrict__ qb, int n, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;     // (frame, pixel, 8-channel group)
    if (idx >= total) return;
    const int g = (int)(idx & 15);
    const int64_t pix = idx >> 4;
    const int frame = (int)(pix / n);
    const f32x4 a = *(const f32x4*)(q + pix * ld + g * 8), b = *(const f32x4*)(q + pix * ld + g * 8 + 4);
    const f32x4 pa = *(const f32x4*)(pe + frame * 128 + g * 8), pb = *(const f32x4*)(pe + frame * 128 + g * 8 + 4);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o[j] = (bf16_t)(a[j] + pa[j]);
        o[4 + j] = (bf16_t)(b[j] + pb[j]);
    }
    *(bf16x8*)(qb + pix * 128 + g * 8) = o;
}
extern "C" int ppms_attn_prep_q(const float* q, int ld, const float* pe, void* qb, int T, int n, void* stream) {
    PPMS_REQUIRE(q && pe && qb && ld % 4 == 0 && T > 0 && n > 0, "attn_prep_q: bad arguments (T, n > 0, ld %% 4 == 0)");
    PPMS_REQUIRE((((uintptr_t)q | (uintptr_t)pe | (uintptr_t)qb) & 15) == 0, "attn_prep_q: q, pe and qb must be 16-byte aligned");
    const int64_t total = (int64_t)T * n * 16;
    hipLaunchKernelGGL(attn_prep_q_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, q, ld, pe, (bf16_t*)qb, n, total);
    return ppms_check_launch("attn_prep_q");
}

__global__ __launch_bounds__(256) void attn_prep_k_kernel(const float* __restrict__ key, int ld, const float* __restrict__ pe,
                                                          const int32_t* __restrict__ sel, const float* __restrict__ shat,
                                                          bf16_t* __restrict__ kb, int ksel, int n, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;     // (clip, slot, pixel, 8-channel group)
    if (idx >= total) return;
    const int g = (int)(idx & 15);
    const int64_t r = idx >> 4;
    const int pin = (int)(r % n);
    const int cs = (int)(r / n);                // clip*ksel + slot
    const int clip = cs / ksel, slot = cs - clip * ksel;
    const int frame = sel[clip * 5 + slot];
    const float s = shat[clip * 5 + slot];
    const float* kp = key + ((int64_t)frame * n + pin) * ld + g * 8;
    const f32x4 a = *(const f32x4*)kp, b = *(const f32x4*)(kp + 4);
    const f32x4 pa = *(const f32x4*)(pe + frame * 128 + g * 8), pb = *(const f32x4*)(pe + frame * 128 + g * 8 + 4);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o[j] = (bf16_t)(a[j] * s + pa[j]);
        o[4 + j] = (bf16_t)(b[j] * s + pb[j]);
    }
    *(bf16x8*)(kb + r * 128 + g * 8) = o;
}
extern "C" int ppms_attn_prep_k(const float* key, int ld, const float* pe, const int32_t* sel, const float* shat, void* kb, int T, int ksel,
                                int n, void* stream) {
    PPMS_REQUIRE(key && pe && sel && shat && kb && ksel >= 1 && ksel <= 5 && ld % 4 == 0 && T > 0 && n > 0,
                 "attn_prep_k: bad arguments (T, n > 0, 1 <= ksel <= 5, ld %% 4 == 0)");
    PPMS_REQUIRE((((uintptr_t)key | (uintptr_t)pe | (uintptr_t)kb) & 15) == 0, "attn_prep_k: key, pe and kb must be 16-byte aligned");
    const int64_t total = (int64_t)T * ksel * n * 16;
    hipLaunchKernelGGL(attn_prep_k_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, key, ld, pe, sel, shat,
                       (bf16_t*)kb, ksel, n, total);
    return ppms_check_launch("attn_prep_k");
}

// QAM pick + key modulation in ONE launch (the loop of an unsharded engine): wave 0 of EVERY workgroup runs the pick (qam_pick, the arithmetic
// of qam_select_kernel) redundantly into LDS and turns it into one list per key frame j of the (clip, slot) pairs that picked j; workgroup 0
// alone stores SEL / SHAT / SCORE and the new usage counter.  The counter is a ping-pong pair: every workgroup reads strive_in, workgroup 0
// writes all of strive_out.  Nothing passes between workgroups.  Modulation: a thread owns (key frame, pixel, 8 channels), loads the fp32 key
// and the PE row once and writes bf16(K s_hat + PE) -- attn_prep_k_kernel's expression -- to every (clip, slot) of the frame's list; a frame
// nobody picked (T > 5) is skipped.  Grid-stride loop; the first key load is issued in front of the pick.
// Dynamic LDS: 3 T T floats -- qam_pick's tables, then (the pick done) the lists: T T (clip * ksel + slot) ints + T T s_hat floats.
__global__ __launch_bounds__(256) void pick_prep_k_kernel(const float* __restrict__ sim, const float* __restrict__ strive_in,
                                                          float* __restrict__ strive_out, const float* __restrict__ partial, int nblk, int HW,
                                                          int32_t* __restrict__ sel_g, float* __restrict__ shat_g, float* __restrict__ score_g,
                                                          const float* __restrict__ key, int ld, const float* __restrict__ pe,
                                                          bf16_t* __restrict__ kb, int T, int n) {
    extern __shared__ __attribute__((aligned(16))) char pick_smem[];
    __shared__ float conf[64];
    __shared__ int32_t sel_s[64 * 5];
    __shared__ float shat_s[64 * 5];
    __shared__ unsigned long long mask_s[64];
    __shared__ int lcnt[64];
    int* lcs = (int*)pick_smem;                          // [frame][k]: clip * ksel + slot
    float* lsh = (float*)pick_smem + T * T;              // [frame][k]: s_hat of that pair
    const int tid = threadIdx.x, ksel = T < 5 ? T : 5;
    const bool first = blockIdx.x == 0, wave0 = tid < 64;
    const int64_t total = (int64_t)T * n * 16, stride = (int64_t)gridDim.x * 256;     // (key frame, pixel, 8-channel group)
    int64_t idx = (int64_t)blockIdx.x * 256 + tid;
    f32x4 a = {0, 0, 0, 0}, b = {0, 0, 0, 0};
    if (idx < total) {
        const float* kp = key + (idx >> 4) * ld + (idx & 15) * 8;
        a = *(const f32x4*)kp;
        b = *(const f32x4*)(kp + 4);
    }
    const unsigned long long picked = qam_pick(sim, strive_in, first ? strive_out : nullptr, partial, nblk, HW, sel_s, shat_s,
                                               first ? score_g : nullptr, T, conf, (float*)pick_smem, wave0, tid);
    if (wave0 && tid < T) mask_s[tid] = picked;
    __syncthreads();                                     // (the tables are dead: the lists take their place)
    if (wave0 && tid < T) {                              // lane j: who picked frame j, in clip order; sel is ascending, so the slot is a bit count
        int cnt = 0;
        for (int i = 0; i < T; ++i) {
            const unsigned long long m = mask_s[i];
            if ((m >> tid) & 1ull) {
                const int s = __popcll(m & ((1ull << tid) - 1ull));
                lcs[tid * T + cnt] = i * ksel + s;
                lsh[tid * T + cnt] = shat_s[i * 5 + s];
                ++cnt;
            }
        }
        lcnt[tid] = cnt;
        if (first)
            for (int s = 0; s < 5; ++s) {
                sel_g[tid * 5 + s] = sel_s[tid * 5 + s];
                shat_g[tid * 5 + s] = shat_s[tid * 5 + s];
            }
    }
    __syncthreads();
    while (idx < total) {
        const int64_t nidx = idx + stride;
        f32x4 na = {0, 0, 0, 0}, nb = {0, 0, 0, 0};
        if (nidx < total) {
            const float* kp = key + (nidx >> 4) * ld + (nidx & 15) * 8;
            na = *(const f32x4*)kp;
            nb = *(const f32x4*)(kp + 4);
        }
        const int g = (int)(idx & 15);
        const int64_t r = idx >> 4;
        const int frame = (int)(r / n);
        const int pin = (int)(r - (int64_t)frame * n);
        const int cnt = lcnt[frame];
        if (cnt > 0) {
            const f32x4 pa = *(const f32x4*)(pe + frame * 128 + g * 8), pb = *(const f32x4*)(pe + frame * 128 + g * 8 + 4);
            for (int k = 0; k < cnt; ++k) {
                const int cs = lcs[frame * T + k];
                const float s = lsh[frame * T + k];
                bf16x8 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    o[j] = (bf16_t)(a[j] * s + pa[j]);
                    o[4 + j] = (bf16_t)(b[j] * s + pb[j]);
                }
                *(bf16x8*)(kb + ((int64_t)cs * n + pin) * 128 + g * 8) = o;
            }
        }
        a = na;
        b = nb;
        idx = nidx;
    }
}
// strive_in / strive_out: the usage counter before / after this pick (two distinct fp32 [T][T] tables); the other arguments as those of
// ppms_qam_select and ppms_attn_prep_k (sel / shat / kb of all T clips: an unsharded window).
extern "C" int ppms_pick_prep_k(const float* sim, const float* strive_in, float* strive_out, const float* conf_partial, int nblk, int HW,
                                int32_t* sel, float* shat, float* score, const float* key, int ld, const float* pe, void* kb, int T, int n,
                                void* stream) {
    PPMS_REQUIRE(sim && strive_in && strive_out && strive_in != strive_out && conf_partial && sel && shat && T > 0 && T <= 64 && nblk >= 0,
                 "pick_prep_k: bad arguments (1 <= T <= 64, two distinct counter tables)");
    PPMS_REQUIRE(key && pe && kb && n > 0 && ld % 4 == 0, "pick_prep_k: bad key operands");
    PPMS_REQUIRE((((uintptr_t)key | (uintptr_t)pe | (uintptr_t)kb) & 15) == 0, "pick_prep_k: key, pe and kb must be 16-byte aligned");
    const int64_t total = (int64_t)T * n * 16;
    // few, fat workgroups: every workgroup pays the pick once, so all of them are resident at once (a CU holds 8 of these) and each streams
    // several items behind it.  Measured: 2, 4, 8 or 16 per CU give the same clip time (profiles/r08_pick_chain_ab.txt)
    constexpr int PICK_PREP_WG_PER_CU = 4;
    const int64_t cap = (int64_t)ppms_num_cus() * PICK_PREP_WG_PER_CU;
    const int64_t nwg = ceil_div(total, 256) < cap ? ceil_div(total, 256) : cap;
    hipLaunchKernelGGL(pick_prep_k_kernel, dim3((unsigned)nwg), dim3(256), (size_t)T * T * 12, (hipStream_t)stream, sim, strive_in, strive_out,
                       conf_partial, nblk, HW, sel, shat, score, key, ld, pe, (bf16_t*)kb, T, n);
    return ppms_check_launch("pick_prep_k");
}
