// profile.hip - per-family launch timing (HIP events on the launch stream): ProfScope and the icd_profile_* entries.
#include <algorithm>
#include <vector>
#include "profile.h"

namespace {

struct ProfRec { hipEvent_t a, b; int kind; double flops, bytes; int M, N, K, aux; int tile_m, tile_n, plan_flags, ksplit; double xflops; };
bool g_prof_on = false;
unsigned g_prof_mask = 0xffffffffu;     // bit k: record launches of family k
std::vector<ProfRec> g_prof;
std::vector<hipEvent_t> g_ev_pool;

hipEvent_t prof_event() {
    if (!g_ev_pool.empty()) { hipEvent_t e = g_ev_pool.back(); g_ev_pool.pop_back(); return e; }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}

}  // namespace

ProfScope::ProfScope(hipStream_t s, int kind, double flops, double bytes, int M, int N, int K, int aux)
    : on(g_prof_on && ((g_prof_mask >> kind) & 1u)), st(s), idx(0) {
    if (!on) return;
    ProfRec r{prof_event(), prof_event(), kind, flops, bytes, M, N, K, aux, 0, 0, 0, 0, flops};
    (void)hipEventRecord(r.a, st);
    idx = g_prof.size();
    g_prof.push_back(r);
}
ProfScope::~ProfScope() { if (on) (void)hipEventRecord(g_prof[idx].b, st); }
void ProfScope::executed(double xf) { if (on) g_prof[idx].xflops = xf; }
void ProfScope::plan(const icd_gemm_desc& d) {
    if (!on) return;
    icd_gemm_plan_info pi;
    if (icd_gemm_plan(&d, &pi) != ICD_OK) return;
    ProfRec& r = g_prof[idx];
    r.tile_m = pi.tile_m; r.tile_n = pi.tile_n; r.ksplit = pi.ksplit;
    r.plan_flags = (pi.kernel ? 1 : 0) | (pi.ln_inline ? 2 : 0) | (pi.xattn ? 4 : 0);
}

extern "C" int icd_profile_enable(int32_t enable) {
    for (auto& r : g_prof) { g_ev_pool.push_back(r.a); g_ev_pool.push_back(r.b); }
    g_prof.clear();
    g_prof_on = enable != 0;
    g_prof_mask = enable > 0 ? 0xffffffffu : (unsigned)(-enable);     // enable < 0: bit mask of the families to record
    return ICD_OK;
}

extern "C" int icd_profile_read(icd_profile_row* rows, int32_t max_rows) {
    ICD_CHECK_ARG(rows && max_rows >= ICD_PROF_KINDS, "icd_profile_read: need room for %d rows", ICD_PROF_KINDS);
    for (int k = 0; k < ICD_PROF_KINDS; ++k) { rows[k].kind = k; rows[k].launches = 0; rows[k].ms = rows[k].flops = rows[k].bytes = rows[k].flops_executed = 0.0; }
    for (auto& r : g_prof) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) { icd_set_error("icd_profile_read: events not complete (synchronise the stream first)"); return ICD_ERR_HIP; }
        rows[r.kind].launches += 1; rows[r.kind].ms += ms; rows[r.kind].flops += r.flops; rows[r.kind].bytes += r.bytes;
        rows[r.kind].flops_executed += r.xflops;
    }
    return ICD_PROF_KINDS;
}

extern "C" int icd_profile_dump(icd_profile_record* recs, int32_t max_recs) {
    const int n = (int)std::min<size_t>(g_prof.size(), (size_t)std::max(0, max_recs));
    for (int i = 0; i < n && recs; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, g_prof[i].a, g_prof[i].b) != hipSuccess) { icd_set_error("icd_profile_dump: events not complete"); return ICD_ERR_HIP; }
        recs[i].kind = g_prof[i].kind; recs[i].M = g_prof[i].M; recs[i].N = g_prof[i].N; recs[i].K = g_prof[i].K; recs[i].aux = g_prof[i].aux;
        recs[i].ms = ms; recs[i].flops = g_prof[i].flops;
        recs[i].tile_m = g_prof[i].tile_m; recs[i].tile_n = g_prof[i].tile_n; recs[i].plan_flags = g_prof[i].plan_flags; recs[i].ksplit = g_prof[i].ksplit;
    }
    return recs ? n : (int)g_prof.size();
}
