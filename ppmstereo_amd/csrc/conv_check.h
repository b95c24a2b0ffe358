// The ppms_conv descriptor contract of the five convolution kernels, written once (host code only).
//
// Every kernel file holds one ConvRules record and calls the two tiers below from its rating function(s) AND its launch entry point, followed by
// its own geometry planner (plan2 / plan5 / plan6 / plan1 / plan7: the limits only that kernel has).  So a non-zero rating, plus a descriptor
// that passes the operand tier, means the launch takes the descriptor (include/ppms.h).
//   shape / addressing tier (conv_check_shape):  everything a rating may rely on -- it never looks at w, bias or n_valid;
//   operand tier (conv_check_operands):          what only a launch needs.
// A refusal leaves "<kernel>: <field>=<value> ..." in ppms_last_error() and returns false.
#pragma once
#include "common.h"

namespace {

struct ConvRules {
    const char* name;              // kernel name in messages
    int chunk;                     // input segments: channels in multiples of this
    int m_mult;                    // M: a multiple of this; 0: M in {128, 192, 256}
    int split_mult;                // m_split (when < M: two epilogue halves): a multiple of this
    int kt_max, kh_max, kw_max;    // odd taps up to these; 0: no limit
    bool grouped, out_vt, addf32;  // serves groups == 2 / epilogues with out_vt / PPMS_EPI_ADDF32
    int ld_max;                    // segment ld limit; 0: none
};

#define CONV_REFUSE_IF(cond, ...)        \
    do {                                 \
        if (cond) {                      \
            ppms_set_error(__VA_ARGS__); \
            return false;                \
        }                                \
    } while (0)

inline bool conv_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int conv_halves(const ppms_conv* d) { return d->m_split < d->M ? 2 : 1; }      // live epilogue halves
inline bool conv_has_out_vt(const ppms_conv* d) {
    return d->epi[0].out_vt != nullptr || (conv_halves(d) == 2 && d->epi[1].out_vt != nullptr);
}

inline bool conv_check_shape(const ConvRules& r, const ppms_conv* d) {
    const char* k = r.name;
    CONV_REFUSE_IF(d == nullptr, "%s: null descriptor", k);
    CONV_REFUSE_IF(d->nseg != 1 && d->nseg != 2, "%s: nseg=%d (1 or 2)", k, d->nseg);
    if (r.grouped) CONV_REFUSE_IF(d->groups < 0 || d->groups > 2, "%s: groups=%d (0, 1 or 2)", k, d->groups);
    else CONV_REFUSE_IF(d->groups < 0 || d->groups > 1, "%s: a grouped convolution (groups=%d) is served by ppms_conv_gemm6 only", k, d->groups);
    CONV_REFUSE_IF(d->T <= 0 || d->H <= 0 || d->W <= 0, "%s: bad volume T=%d H=%d W=%d", k, d->T, d->H, d->W);
    CONV_REFUSE_IF(d->t_halo < 0 || d->t_halo > 8, "%s: t_halo=%d (0..8)", k, d->t_halo);
    const int kk[3] = {d->kt, d->kh, d->kw}, kmax[3] = {r.kt_max, r.kh_max, r.kw_max};
    const char* const kn[3] = {"kt", "kh", "kw"};
    for (int a = 0; a < 3; ++a) {
        CONV_REFUSE_IF(kk[a] < 1 || !(kk[a] & 1), "%s: %s=%d must be odd", k, kn[a], kk[a]);
        CONV_REFUSE_IF(kmax[a] && kk[a] > kmax[a], "%s: %s=%d (<= %d)", k, kn[a], kk[a], kmax[a]);
    }
    if (r.m_mult) CONV_REFUSE_IF(d->M <= 0 || d->M % r.m_mult, "%s: M=%d must be a multiple of %d", k, d->M, r.m_mult);
    else CONV_REFUSE_IF(d->M != 128 && d->M != 192 && d->M != 256, "%s: M=%d must be 128, 192 or 256", k, d->M);
    CONV_REFUSE_IF(conv_halves(d) == 2 && d->m_split % r.split_mult, "%s: m_split=%d must be a multiple of %d", k, d->m_split, r.split_mult);
    for (int s = 0; s < d->nseg; ++s) {
        const ppms_sp& sg = d->seg[s];
        CONV_REFUSE_IF(sg.hi == nullptr || sg.lo == nullptr, "%s: seg[%d] needs hi and lo planes", k, s);
        CONV_REFUSE_IF(!conv_al16(sg.hi) || !conv_al16(sg.lo), "%s: seg[%d] planes not 16-B aligned", k, s);
        CONV_REFUSE_IF(sg.c <= 0 || sg.c % r.chunk, "%s: seg[%d].c=%d must be a multiple of %d", k, s, sg.c, r.chunk);
        CONV_REFUSE_IF(sg.ld % 8, "%s: seg[%d].ld=%d must be a multiple of 8", k, s, sg.ld);
        CONV_REFUSE_IF(r.ld_max && sg.ld > r.ld_max, "%s: seg[%d].ld=%d (<= %d)", k, s, sg.ld, r.ld_max);
    }
    for (int h = 0; h < conv_halves(d); ++h) {
        CONV_REFUSE_IF(!r.out_vt && d->epi[h].out_vt != nullptr, "%s: epi[%d].out_vt is not served (ppms_conv_gemm5 / ppms_gemm1 write V^T)", k, h);
        CONV_REFUSE_IF(!r.addf32 && d->epi[h].kind == PPMS_EPI_ADDF32, "%s: epi[%d].kind=ADDF32 is not served", k, h);
    }
    return true;
}

// alignment rules of the coalesced row epilogue (conv_epilogue.h: 8 couts of one pixel per lane, 16-byte accesses)
inline const char* epilogue_row8_check(const ppms_epilogue& e) {
    if (e.out_sp.hi != nullptr && !(conv_al16(e.out_sp.hi) && conv_al16(e.out_sp.lo) && e.out_sp.ld % 8 == 0)) return "out_sp must be 16-byte aligned with ld % 8 == 0";
    if ((e.kind == PPMS_EPI_RESID || e.kind == PPMS_EPI_RH || e.kind == PPMS_EPI_GRU) &&
        !(conv_al16(e.aux_sp.hi) && conv_al16(e.aux_sp.lo) && e.aux_sp.ld % 8 == 0))
        return "aux_sp must be 16-byte aligned with ld % 8 == 0";
    if (e.out_f32 != nullptr && !(conv_al16(e.out_f32) && e.out_f32_ld % 4 == 0)) return "out_f32 must be 16-byte aligned with ld % 4 == 0";
    if (e.kind == PPMS_EPI_GRU && !(conv_al16(e.aux_f32) && e.aux_f32_ld % 4 == 0)) return "aux_f32 must be 16-byte aligned with ld % 4 == 0";
    if (e.pre_f32 != nullptr && !(conv_al16(e.pre_f32) && e.pre_f32_ld % 4 == 0)) return "pre_f32 must be 16-byte aligned with ld % 4 == 0";
    if (e.out_vt != nullptr && (e.kind != PPMS_EPI_STORE || e.pre_f32 != nullptr)) return "out_vt needs a STORE epilogue without pre_f32";
    return nullptr;
}

inline bool conv_check_operands(const ConvRules& r, const ppms_conv* d) {
    const char* k = r.name;
    CONV_REFUSE_IF(d->w == nullptr || d->bias == nullptr, "%s: w/bias missing (w=%p bias=%p)", k, d->w, (const void*)d->bias);
    for (int h = 0; h < conv_halves(d); ++h) {
        const ppms_epilogue& e = d->epi[h];
        CONV_REFUSE_IF(e.n_valid <= 0, "%s: epi[%d].n_valid=%d", k, h, e.n_valid);
        CONV_REFUSE_IF(e.kind < PPMS_EPI_STORE || e.kind > PPMS_EPI_ADDF32, "%s: epi[%d].kind=%d unknown", k, h, e.kind);
        CONV_REFUSE_IF(e.pre_f32 != nullptr && e.n_valid % 4, "%s: epi[%d].n_valid=%d must be a multiple of 4 with pre_f32", k, h, e.n_valid);
        const char* why = epilogue_row8_check(e);
        CONV_REFUSE_IF(why != nullptr, "%s: epi[%d]: %s", k, h, why);
        CONV_REFUSE_IF(e.out_sp.hi != nullptr && e.out_sp.lo == nullptr, "%s: epi[%d].out_sp has no lo plane", k, h);
        const bool aux = e.kind == PPMS_EPI_RESID || e.kind == PPMS_EPI_RH || e.kind == PPMS_EPI_GRU;
        CONV_REFUSE_IF(aux && (e.aux_sp.hi == nullptr || e.aux_sp.lo == nullptr), "%s: epi[%d].aux_sp missing for kind=%d", k, h, e.kind);
        CONV_REFUSE_IF(e.kind == PPMS_EPI_GRU && e.aux_f32 == nullptr, "%s: epi[%d].aux_f32 (z) missing for the GRU epilogue", k, h);
        CONV_REFUSE_IF(e.kind == PPMS_EPI_ADDF32 && e.out_f32 == nullptr, "%s: epi[%d].out_f32 missing for the ADDF32 epilogue", k, h);
    }
    return true;
}

}  // namespace
