// Test hook of the C-ABI (include/crfp_hip.h, crfp_dcn_tail_probe): the fused offset head + DCN launch (dcn_fused.inc) with a warp plan in its
// idle last-round CUs, against the same launch without a plan followed by the stand-alone warp.  No kernel of its own and no tensor conversion:
// every pointer is a device buffer the caller laid out in the build's storage format (the offset feature image, the packed weight images, P4
// planes behind their zeroed guard), and goes into DcnFuseArgs / launch_flow_warp_q4 as Runner::frame (engine.hip) binds them.  The DCN map is
// h x w, the warped map 4h x 4w (the 2x and 8x maps of a frame).  Compiled twice (csrc/Makefile): crfp_dcn_tail_probe and crfp_dcn_tail_probe_bf16.
#include "crfp_common.h"
#include "../../include/crfp_hip.h"
#include <cstring>

using namespace CRFP_NS;

namespace {
void report_of(const crfp_dcn_tail_args& a, crfp_dcn_tail_report* r) {
    const DcnFusedGrid g = dcn_fused_grid(a.n, a.h, a.w);
    memset(r, 0, sizeof(*r));
    r->cus = g.cus; r->tiles = g.tiles; r->persistent = g.persistent;
    r->warp_wgs = dcn_fused_tail_wgs(a.n, a.h, a.w);
    r->plan_taken = a.bands > 0 && r->warp_wgs > 0;
    r->grid = g.persistent ? g.cus : g.tiles + (r->plan_taken ? r->warp_wgs : 0);
}
bool geometry_ok(const crfp_dcn_tail_args* a) {
    if (!a) { set_error("dcn_tail_probe: null argument block"); return false; }
    if (a->n < 1 || a->n > 65535 || a->h < 1 || a->w < 1 || (long long)(4 * (long long)a->h + 1) * (4 * (long long)a->w + 1) >= (1ll << 27) || a->bands < 0 || a->bands > 3) {
        set_error("dcn_tail_probe: bad geometry (n=%d h=%d w=%d bands=%d)", a->n, a->h, a->w, a->bands);
        return false;
    }
    return true;
}
}  // namespace

extern "C" {

int CRFP_API(crfp_dcn_tail_plan)(const crfp_dcn_tail_args* a, crfp_dcn_tail_report* report) {
    if (!report) { set_error("dcn_tail_plan: null result pointer"); return CRFP_E_BADARG; }
    if (!geometry_ok(a)) return CRFP_E_BADARG;
    report_of(*a, report);
    return report->cus > 0 ? 0 : CRFP_E_UNSUPPORTED;
}

int CRFP_API(crfp_dcn_tail_probe)(const crfp_dcn_tail_args* a, crfp_dcn_tail_report* report, void* stream) {
    if (!report) { set_error("dcn_tail_probe: null result pointer"); return CRFP_E_BADARG; }
    if (!geometry_ok(a)) return CRFP_E_BADARG;
    if (!a->feat || !a->flow || !a->wconv || !a->bconv || !a->x || !a->wdcn || !a->bdcn || !a->out || !a->status || !a->warp_src || !a->warp_flow || !a->warp_dst) {
        set_error("dcn_tail_probe: null tensor");
        return CRFP_E_BADARG;
    }
    report_of(*a, report);
    if (report->cus <= 0) return CRFP_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const int H8 = 4 * a->h, W8 = 4 * a->w;
    DcnFuseArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.feat = (const float*)a->feat; fa.feat_b = a->feat_b; fa.flow = (const float*)a->flow; fa.flow_b = a->flow_b;
    fa.wconv = a->wconv; fa.bconv = (const float*)a->bconv;
    fa.x = (const float*)a->x; fa.xb = a->x_b;
    fa.wdcn = (const float*)a->wdcn; fa.bdcn = (const float*)a->bdcn;
    fa.out = (float*)a->out; fa.ob = a->out_b; fa.N = a->n; fa.H = a->h; fa.W = a->w; fa.ovf = a->status; fa.ovf_div = 1;
    if (!report->plan_taken) {   // no plan asked for, or none can be taken: the stand-alone path, whole
        int rc = launch_dcn_fused(fa, s);
        if (!rc) rc = launch_flow_warp_q4((const float*)a->warp_src, a->warp_src_b, (const float*)a->warp_flow, a->warp_flow_b, (float*)a->warp_dst, a->warp_dst_b,
                                          a->n, 1, H8, W8, 0, 1, s);
        return rc;
    }
    for (int b = 0; b < a->bands; ++b) {   // one fused launch per band, as the levels of a frame carry them
        fa.warp.src = (const float*)a->warp_src; fa.warp.src_b = a->warp_src_b; fa.warp.flow = (const float*)a->warp_flow; fa.warp.flow_b = a->warp_flow_b;
        fa.warp.dst = (float*)a->warp_dst; fa.warp.dst_b = a->warp_dst_b; fa.warp.H8 = H8; fa.warp.W8 = W8;
        fa.warp.band(b, a->bands);
        const int rc = launch_dcn_fused(fa, s);
        if (rc) return rc;
    }
    return 0;
}

}  // extern "C"
