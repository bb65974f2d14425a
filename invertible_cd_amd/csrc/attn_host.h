// attn_host.h - host side of the attention entries (attention.hip, attention_masked.hip, attention_wide.hip): every entry is validate -> plan -> launch.
// *_validate holds every refusal; *_plan is a pure function of shape and flags that names one row of its kernel family's table of
// instantiations; *_launch turns the row into the instantiation.  The plan is the struct icd_attention_plan reports.  No device code.
#pragma once
#include <utility>
#include "common.h"

typedef icd_attention_info AttnPlan;
enum AttnFamily { ATTN_TILED = 0, ATTN_CROSS = 1, ATTN_PROBS = 2, ATTN_MASKED = 3, ATTN_WIDE = 4 };

struct AttnArgs {             // what icd_attention_fused_ex, icd_attention_masked and icd_attention_wide all take
    const void *q, *k, *vt;
    void* out;
    int32_t B, H, Nq, Nk, d, ldq, ldk, ldvt, ldo;
    int64_t vt_bs;
    float scale;
};

// the refusals those entries share, under the entry's name
inline int attn_check_common(const char* name, const AttnArgs& a) {
    ICD_CHECK_ARG(a.q && a.k && a.vt && a.out, "%s: null pointer", name);
    ICD_CHECK_ARG(a.B > 0 && a.H > 0 && a.Nq > 0 && a.Nk > 0, "%s: empty shape", name);
    ICD_CHECK_ARG(a.scale > 0.f, "%s: scale must be positive", name);
    ICD_CHECK_ARG(a.ldq % 8 == 0 && a.ldk % 8 == 0 && a.ldvt % 8 == 0 && a.ldo % 4 == 0 && a.ldvt >= a.Nk,
                  "%s: leading dims must be 16-byte aligned and ldvt >= Nk", name);
    // (a sliced tensor with an odd element offset must be an error here, not a misaligned vector load in the kernel)
    const long long hd = (long long)a.H * a.d;
    ICD_CHECK_ARG(a.ldq >= hd && a.ldk >= hd && a.ldo >= hd, "%s: ldq, ldk and ldo must be >= H * d", name);
    ICD_CHECK_ARG(a.vt_bs == 0 || a.vt_bs >= hd * a.ldvt, "%s: vt_batch_stride below H * d * ldvt", name);
    ICD_CHECK_ARG(((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.vt) % 16 == 0 && (uintptr_t)a.out % 8 == 0,
                  "%s: q, k and vt must be 16-byte aligned, out 8-byte", name);
    return ICD_OK;
}

// icd_attention_masked's validate + plan (attention_masked.hip), also behind icd_attention_plan
int attn_masked_decide(const AttnArgs& a, const int32_t* key_counts, AttnPlan* p);
// icd_attention_wide's validate + plan (attention_wide.hip), also behind icd_attention_plan
int attn_wide_decide(const AttnArgs& a, AttnPlan* p);

// launch(std::integral_constant<int, row>) for the row of a table of N: one compile-time expansion over the table
template <typename F, size_t... I>
int attn_launch_row(int row, F&& launch, std::index_sequence<I...>) {
    int rc = ICD_ERR_UNSUPPORTED;
    (void)((row == (int)I && ((rc = launch(std::integral_constant<int, (int)I>{})), true)) || ...);
    return rc;
}
