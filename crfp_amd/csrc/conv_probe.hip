// Test hook of the C-ABI (include/crfp_hip.h, crfp_conv_probe): ONE launch of the engines' own MFMA conv kernels on caller-supplied
// tensors.  No kernel of its own: the plan comes from add_mfma / plan_sources, the weight images from pack_items (launch_conv_pack +
// launch_conv_pack_split), the tensors are bound with bind_conv and the launch goes through launch_conv_mfma / launch_conv_mfma_dual /
// launch_conv_pair, exactly as an engine's -- what differs is where the tensors live: in the caller's workspace, converted from and to
// NCHW fp32 by this namespace's launch_nchw_to_q4 / launch_q4_to_nchw, so that the storage type is the build's.  Compiled twice
// (csrc/Makefile): crfp_conv_probe and crfp_conv_probe_bf16.
#include "engine_host.h"

namespace CRFP_NS {
namespace {

constexpr int kMaxCh = 4096, kMaxN = 65535;

struct Bump {   // 256-byte aligned pieces of the workspace; base == null: sizes only
    char* base;
    size_t off = 0;
    char* take(size_t bytes) {
        off = align_up(off, 256);
        char* p = base ? base + off : nullptr;
        off += bytes;
        return p;
    }
};

struct ProbeConv {   // one conv of a call: its plan item, its device tensors, the launch-time plan
    const crfp_probe_conv* c = nullptr;
    Item it;
    int cin = 0, ncq = 0;
    float* src[CRFP_PROBE_MAX_SRC] = {};
    size_t src_bytes[CRFP_PROBE_MAX_SRC] = {};
    float* resid = nullptr;
    float* dst[CRFP_PROBE_MAX_DST] = {};
    size_t dst_bytes[CRFP_PROBE_MAX_DST] = {};
    int dst_ch[CRFP_PROBE_MAX_DST] = {};
    float* s3 = nullptr;       // S3 chain: conv a's only output, conv b's only source
    ConvArgs plan;
};

struct Probe {
    int mode = 0, n = 0, h = 0, w = 0, count = 0;
    ProbeConv cv[2];
    float* packed = nullptr;
    size_t packed_floats = 0;
    unsigned* status = nullptr;
    size_t bytes = 0;
};

bool own_sources(int mode, int k) { return k == 0 || mode == CRFP_PROBE_DUAL; }

int check_conv(const crfp_probe_conv& c, const char* who, int mode, int k, bool need_ptrs) {
    const bool srcs = own_sources(mode, k);
    if (srcs && (c.nsrc < 1 || c.nsrc > CRFP_PROBE_MAX_SRC)) { set_error("conv_probe %s: 1 .. %d sources (got %d)", who, CRFP_PROBE_MAX_SRC, c.nsrc); return CRFP_E_BADARG; }
    for (int i = 0; srcs && i < c.nsrc; ++i) {
        const int kind = c.src_kind[i], nch = c.src_nch[i], pad = c.src_pad[i];
        if (kind != CRFP_PROBE_SRC_Q4 && kind != CRFP_PROBE_SRC_UNSHUF4 && kind != CRFP_PROBE_SRC_FLOW2) { set_error("conv_probe %s: source %d of unknown kind %d", who, i, kind); return CRFP_E_BADARG; }
        if (nch < 1 || nch > kMaxCh || (kind == CRFP_PROBE_SRC_FLOW2 && nch != 2) || (kind == CRFP_PROBE_SRC_UNSHUF4 && nch % 16)) {
            set_error("conv_probe %s: source %d has %d channels (flow: 2, pixel_unshuffle(4): a multiple of 16)", who, i, nch);
            return CRFP_E_BADARG;
        }
        if (pad != 0 && !(pad == 1 && kind == CRFP_PROBE_SRC_Q4)) { set_error("conv_probe %s: source %d: only Q4 sources come in padded planes (pad = %d)", who, i, pad); return CRFP_E_BADARG; }
        if (need_ptrs && !c.src[i]) { set_error("conv_probe %s: null source %d", who, i); return CRFP_E_BADARG; }
    }
    if (c.cout < 1 || c.cout > kMaxCh) { set_error("conv_probe %s: cout %d", who, c.cout); return CRFP_E_BADARG; }
    if (c.act < CRFP_ACT_NONE || c.act > CRFP_ACT_SIGMOID) { set_error("conv_probe %s: unknown activation %d", who, c.act); return CRFP_E_BADARG; }
    if (need_ptrs && (!c.weight || !c.bias)) { set_error("conv_probe %s: null weight or bias", who); return CRFP_E_BADARG; }
    const bool second = c.cout_split > 0;
    if (second && (c.cout_split >= c.cout || (need_ptrs && (!c.weight2 || !c.bias2)))) { set_error("conv_probe %s: cout_split %d needs 0 < cout_split < cout and weight2 / bias2", who, c.cout_split); return CRFP_E_BADARG; }
    const int ncq = (conv_packed_rows(c.cout, c.store, c.ps_r) + 3) / 4;
    const int min_dst = (k == 0 && (mode == CRFP_PROBE_PAIR || mode == CRFP_PROBE_PAIR_F32 || mode == CRFP_PROBE_S3_CHAIN)) ? 0 : 1;
    switch (c.store) {
        case CRFP_PROBE_ST_Q4:
            if (c.ndst < min_dst || c.ndst > CRFP_PROBE_MAX_DST) { set_error("conv_probe %s: %d destinations", who, c.ndst); return CRFP_E_BADARG; }
            for (int d = 0; d < c.ndst; ++d) {
                if (c.dst_q0[d] < 0 || c.dst_q1[d] <= c.dst_q0[d] || c.dst_q1[d] > ncq || (c.dst_pad[d] != 0 && c.dst_pad[d] != 1)) {
                    set_error("conv_probe %s: destination %d takes quads [%d, %d) of %d, pad %d", who, d, c.dst_q0[d], c.dst_q1[d], ncq, c.dst_pad[d]);
                    return CRFP_E_BADARG;
                }
                if (need_ptrs && !c.dst[d]) { set_error("conv_probe %s: null destination %d", who, d); return CRFP_E_BADARG; }
            }
            if (c.dst_f32 && (c.ndst != 1 || c.dst_q0[0] != 0 || c.dst_q1[0] != ncq)) { set_error("conv_probe %s: dst_f32 takes one destination with every quad", who); return CRFP_E_BADARG; }
            break;
        case CRFP_PROBE_ST_PS:
            if ((c.ps_r != 2 && c.ps_r != 4) || c.cout % (c.ps_r * c.ps_r) || c.residual || c.ndst != 1 || c.dst_pad[0] || c.dst_f32 || (need_ptrs && !c.dst[0])) {
                set_error("conv_probe %s: a pixel-shuffle store takes r in {2, 4}, cout %% r^2 == 0, no residual, one unpadded destination", who);
                return CRFP_E_BADARG;
            }
            break;
        case CRFP_PROBE_ST_OFFMASK:
            if ((c.cout & 3) || c.n_off_quads < 0 || c.n_off_quads > c.cout / 4 || c.residual || c.ndst != 1 || c.dst_pad[0] || (need_ptrs && (!c.flow || !c.dst[0]))) {
                set_error("conv_probe %s: an offset / mask store takes cout %% 4 == 0, 0 <= n_off_quads <= cout / 4, a flow field, no residual, one unpadded destination", who);
                return CRFP_E_BADARG;
            }
            break;
        default: set_error("conv_probe %s: unknown store mode %d", who, c.store); return CRFP_E_BADARG;
    }
    return 0;
}

// validates the call, builds both plan items and lays the workspace out behind `base` (null: sizes only, plans unbound)
int prepare(Probe& P, int mode, const crfp_probe_conv* a, const crfp_probe_conv* b, int n, int h, int w, char* base, bool need_ptrs) {
    if (mode < CRFP_PROBE_SINGLE || mode > CRFP_PROBE_PAIR_F32) { set_error("conv_probe: unknown mode %d", mode); return CRFP_E_BADARG; }
    if (!a || (mode != CRFP_PROBE_SINGLE && !b)) { set_error("conv_probe: null conv descriptor"); return CRFP_E_BADARG; }
    if (n < 1 || n > kMaxN || h < 1 || w < 1 || (long long)h * w > (1LL << 24)) { set_error("conv_probe: bad geometry (n=%d h=%d w=%d)", n, h, w); return CRFP_E_BADARG; }
    if (mode == CRFP_PROBE_PAIR && !kActBf16) { set_error("conv_probe: the pair kernel exists in the bf16 build only"); return CRFP_E_UNSUPPORTED; }
    if (mode == CRFP_PROBE_PAIR_F32 && kActBf16) { set_error("conv_probe: the fp32 pair kernel exists in the fp32 build only"); return CRFP_E_UNSUPPORTED; }
    if (mode == CRFP_PROBE_S3_CHAIN && kActBf16) { set_error("conv_probe: SRC_S3 images exist in the fp32 build only"); return CRFP_E_UNSUPPORTED; }
    P.mode = mode; P.n = n; P.h = h; P.w = w;
    P.count = mode == CRFP_PROBE_SINGLE ? 1 : 2;
    P.cv[0].c = a; P.cv[1].c = b;
    for (int k = 0; k < P.count; ++k) {
        const int rc = check_conv(*P.cv[k].c, k ? "b" : "a", mode, k, need_ptrs);
        if (rc) return rc;
    }
    if (mode == CRFP_PROBE_S3_CHAIN && (a->store != CRFP_PROBE_ST_Q4 || (a->cout & 15))) {
        set_error("conv_probe: an S3 chain needs conv a to store ST_Q4 with cout %% 16 == 0 (got %d)", a->cout);
        return CRFP_E_BADARG;
    }
    Bump B{base};
    Item items[2];
    for (int k = 0; k < P.count; ++k) {
        ProbeConv& v = P.cv[k];
        const crfp_probe_conv& c = *v.c;
        std::vector<SrcSpec> specs;
        if (own_sources(mode, k)) for (int i = 0; i < c.nsrc; ++i) specs.push_back({c.src_kind[i], c.src_nch[i]});
        else specs.push_back({mode == CRFP_PROBE_S3_CHAIN ? (int)SRC_S3 : (int)SRC_Q4, a->cout});
        for (auto& s : specs) v.cin += s.nch;
        if (v.cin > kMaxCh) { set_error("conv_probe: %d input channels", v.cin); return CRFP_E_BADARG; }
        add_mfma(items[k], k ? "conv_probe:b" : "conv_probe:a", 2 * k, c.cout_split > 0 ? 2 * k + 1 : -1, v.cin, c.cout, specs, c.store, c.ps_r, c.act, c.post_scale);
        items[k].c.n_off_quads = c.n_off_quads;
        v.ncq = (conv_packed_rows(c.cout, c.store, c.ps_r) + 3) / 4;
    }
    P.packed_floats = assign_offsets(items, P.count);
    P.packed = (float*)B.take(P.packed_floats * sizeof(float));
    P.status = (unsigned*)B.take(2 * (size_t)n * sizeof(unsigned));
    const size_t px = (size_t)h * w;
    for (int k = 0; k < P.count; ++k) {
        ProbeConv& v = P.cv[k];
        const crfp_probe_conv& c = *v.c;
        v.it = items[k];
        if (own_sources(mode, k)) {
            for (int i = 0; i < c.nsrc; ++i) {
                const int nq = (c.src_nch[i] + 3) / 4, pad = c.src_pad[i];
                if (c.src_kind[i] == CRFP_PROBE_SRC_Q4) v.src_bytes[i] = (size_t)n * nq * (h + pad) * (w + pad) * kQuadBytes;
                else if (c.src_kind[i] == CRFP_PROBE_SRC_UNSHUF4) v.src_bytes[i] = (size_t)n * ((c.src_nch[i] / 16 + 3) / 4) * 16 * px * kQuadBytes;
                if (v.src_bytes[i]) v.src[i] = (float*)B.take(v.src_bytes[i]);
            }
        } else if (mode == CRFP_PROBE_S3_CHAIN) {
            P.cv[0].s3 = (float*)B.take((size_t)n * (a->cout / 4) * px * 16);
        }
        if (c.residual) v.resid = (float*)B.take((size_t)n * v.ncq * px * kQuadBytes);
        for (int d = 0; d < c.ndst; ++d) {
            const bool fdst = c.store == CRFP_PROBE_ST_OFFMASK || c.dst_f32;
            const size_t qb = fdst ? 16 : kQuadBytes;
            if (c.store == CRFP_PROBE_ST_PS) {
                v.dst_ch[d] = c.cout / (c.ps_r * c.ps_r);
                v.dst_bytes[d] = (size_t)n * ((v.dst_ch[d] + 3) / 4) * px * c.ps_r * c.ps_r * qb;
            } else {
                const int q0 = c.store == CRFP_PROBE_ST_Q4 ? c.dst_q0[d] : 0, q1 = c.store == CRFP_PROBE_ST_Q4 ? c.dst_q1[d] : v.ncq;
                const int pad = c.store == CRFP_PROBE_ST_Q4 ? c.dst_pad[d] : 0;
                v.dst_ch[d] = (4 * q1 < c.cout ? 4 * q1 : c.cout) - 4 * q0;
                v.dst_bytes[d] = (size_t)n * (q1 - q0) * (h + pad) * (w + pad) * qb;
            }
            v.dst[d] = (float*)B.take(v.dst_bytes[d]);
        }
    }
    P.bytes = align_up(B.off, 256);
    return 0;
}

// the launch-time plans: bind_conv, then what the engines set by hand (engine.hip, Run::plan / Run::mfma)
void bind(Probe& P, const float* packed) {
    const int n = P.n, h = P.h, w = P.w;
    const long long px = (long long)h * w;
    for (int k = 0; k < P.count; ++k) {
        ProbeConv& v = P.cv[k];
        const crfp_probe_conv& c = *v.c;
        std::vector<SrcBind> srcs;
        std::vector<DstBind> dsts;
        if (own_sources(P.mode, k)) {
            for (int i = 0; i < c.nsrc; ++i) {
                const long long nq = (c.src_nch[i] + 3) / 4, pad = c.src_pad[i];
                if (c.src_kind[i] == CRFP_PROBE_SRC_Q4) srcs.push_back({v.src[i], nq * (h + pad) * (w + pad) * 4, (int)pad});
                else if (c.src_kind[i] == CRFP_PROBE_SRC_UNSHUF4) srcs.push_back({v.src[i], (long long)((c.src_nch[i] / 16 + 3) / 4) * 16 * px * 4, 0});
                else srcs.push_back({c.src[i], px * 2, 0});
            }
        } else if (P.mode == CRFP_PROBE_S3_CHAIN) {
            srcs.push_back({P.cv[0].s3, (long long)(P.cv[0].c->cout / 4) * px * 4, 0});
        } else {
            srcs.push_back({nullptr, 0, 0});   // the pair kernel keeps the tensor between its convs in LDS
        }
        for (int d = 0; d < c.ndst; ++d) {
            if (c.store == CRFP_PROBE_ST_PS) dsts.push_back({v.dst[d], (long long)((v.dst_ch[d] + 3) / 4) * px * c.ps_r * c.ps_r * 4, 0, (v.dst_ch[d] + 3) / 4, 0});
            else if (c.store == CRFP_PROBE_ST_OFFMASK) dsts.push_back({v.dst[d], (long long)v.ncq * px * 4, 0, v.ncq, 0});
            else dsts.push_back({v.dst[d], (long long)(c.dst_q1[d] - c.dst_q0[d]) * (h + c.dst_pad[d]) * (w + c.dst_pad[d]) * 4, c.dst_q0[d], c.dst_q1[d], c.dst_pad[d]});
        }
        ConvArgs& p = v.plan;
        p = bind_conv(v.it, packed, n, h, w, srcs, dsts, P.status ? P.status + (size_t)k * n : nullptr);
        p.ovf_div = 1; p.ovf_add = 0;   // every batch item its own status word
        p.strict = c.strict;
        p.dst_f32 = c.dst_f32;
        if (c.store == CRFP_PROBE_ST_PS) { p.dstH = h * c.ps_r; p.dstW = w * c.ps_r; }
        p.resid = v.resid; p.resid_bstride = (long long)v.ncq * px * 4;
        p.flow = c.flow; p.flow_bstride = px * 2;
        if (k == 0 && P.mode == CRFP_PROBE_S3_CHAIN) { p.s3_dst = v.s3; p.s3_bstride = (long long)(c.cout / 4) * px * 4; }
    }
}

void choose(const Probe& P, int* kernel) {
    kernel[0] = kernel[1] = CK_NONE;
    if (P.mode == CRFP_PROBE_PAIR) { kernel[0] = kernel[1] = CK_BF16_PAIR; return; }
    if (P.mode == CRFP_PROBE_PAIR_F32) { kernel[0] = kernel[1] = CK_SPLIT_PAIR; return; }
    if (P.mode == CRFP_PROBE_DUAL && conv_select_dual(P.cv[0].plan, P.cv[1].plan) == CK_SPLIT_DUAL) { kernel[0] = kernel[1] = CK_SPLIT_DUAL; return; }
    for (int k = 0; k < P.count; ++k) kernel[k] = conv_select_kernel(P.cv[k].plan);
}

}  // namespace
}  // namespace CRFP_NS

using namespace CRFP_NS;

extern "C" {

size_t CRFP_API(crfp_conv_probe_workspace_bytes)(int mode, const crfp_probe_conv* a, const crfp_probe_conv* b, int n, int h, int w) {
    Probe P;
    return prepare(P, mode, a, b, n, h, w, nullptr, false) ? 0 : P.bytes;
}

int CRFP_API(crfp_conv_probe_kernel)(int mode, const crfp_probe_conv* a, const crfp_probe_conv* b, int n, int h, int w, int* kernel) {
    if (!kernel) { set_error("conv_probe_kernel: null result pointer"); return CRFP_E_BADARG; }
    Probe P;
    const int rc = prepare(P, mode, a, b, n, h, w, nullptr, false);
    if (rc) return rc;
    bind(P, reinterpret_cast<const float*>(256));   // the rule asks whether the weight images exist, never what they hold
    choose(P, kernel);
    return 0;
}

int CRFP_API(crfp_conv_probe)(int mode, const crfp_probe_conv* a, const crfp_probe_conv* b, int n, int h, int w, unsigned* status, int* kernel,
                              void* workspace, size_t workspace_bytes, void* stream) {
    if (!status || !kernel) { set_error("conv_probe: null status or kernel pointer"); return CRFP_E_BADARG; }
    Probe P;
    int rc = prepare(P, mode, a, b, n, h, w, (char*)workspace, true);
    if (rc) return rc;
    if (!workspace || workspace_bytes < P.bytes) { set_error("conv_probe: workspace too small"); return CRFP_E_WORKSPACE; }
    hipStream_t s = (hipStream_t)stream;
    auto fill = [&](void* p, int byte, size_t bytes) {
        if (!rc && bytes && hipMemsetAsync(p, byte, bytes, s) != hipSuccess) { set_error("conv_probe: memset failed"); rc = 1; }
    };
    auto copy = [&](void* dst, const void* src, size_t bytes) {
        if (!rc && hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) { set_error("conv_probe: copy failed"); rc = 1; }
    };
    fill(P.status, 0, 2 * (size_t)n * sizeof(unsigned));
    // weights: the engines' pack loop over this call's one or two items
    const float* params[8] = {};
    Item items[2];
    for (int k = 0; k < P.count; ++k) {
        const crfp_probe_conv& c = *P.cv[k].c;
        params[4 * k] = c.weight; params[4 * k + 1] = c.bias; params[4 * k + 2] = c.weight2; params[4 * k + 3] = c.bias2;
        items[k] = P.cv[k].it;
    }
    RUN(pack_items(items, P.count, params, [&](int ci) { return P.cv[ci / 2].c->cout_split; }, P.packed, s));
    // tensors in: sources and residual in the storage type, destinations poisoned
    for (int k = 0; k < P.count; ++k) {
        ProbeConv& v = P.cv[k];
        const crfp_probe_conv& c = *v.c;
        if (own_sources(mode, k))
            for (int i = 0; i < c.nsrc; ++i) {
                if (c.src_kind[i] == CRFP_PROBE_SRC_Q4) {
                    if (c.src_pad[i]) fill(v.src[i], 0, v.src_bytes[i]);
                    RUN(launch_nchw_to_q4(c.src[i], v.src[i], n, c.src_nch[i], h, w, c.src_pad[i], s));
                } else if (c.src_kind[i] == CRFP_PROBE_SRC_UNSHUF4) {
                    RUN(launch_nchw_to_q4(c.src[i], v.src[i], n, c.src_nch[i] / 16, 4 * h, 4 * w, 0, s));
                }
            }
        if (v.s3) fill(v.s3, 0xFF, (size_t)n * (c.cout / 4) * h * w * 16);
        if (c.residual) RUN(launch_nchw_to_q4(c.residual, v.resid, n, c.cout, h, w, 0, s));
        for (int d = 0; d < c.ndst; ++d) fill(v.dst[d], 0xFF, v.dst_bytes[d]);
    }
    if (rc) return rc;
    bind(P, P.packed);
    choose(P, kernel);
    switch (mode) {
        case CRFP_PROBE_DUAL: rc = launch_conv_mfma_dual(P.cv[0].plan, "conv_probe:a", P.cv[1].plan, "conv_probe:b", "conv_probe:dual", s); break;
        case CRFP_PROBE_PAIR:
#ifdef CRFP_ACT_BF16
            rc = launch_conv_pair(P.cv[0].plan, P.cv[1].plan, "conv_probe:pair", s);
#endif
            break;
        case CRFP_PROBE_PAIR_F32:
#ifndef CRFP_ACT_BF16
            rc = launch_conv_pair(P.cv[0].plan, P.cv[1].plan, "conv_probe:pair", s);
#endif
            break;
        case CRFP_PROBE_S3_CHAIN:
            rc = launch_conv_mfma(P.cv[0].plan, "conv_probe:a", s);
            RUN(launch_conv_mfma(P.cv[1].plan, "conv_probe:b", s));
            break;
        default: rc = launch_conv_mfma(P.cv[0].plan, "conv_probe:a", s);
    }
    // tensors out
    for (int k = 0; k < P.count; ++k) {
        ProbeConv& v = P.cv[k];
        const crfp_probe_conv& c = *v.c;
        for (int d = 0; d < c.ndst; ++d) {
            const bool fdst = c.store == CRFP_PROBE_ST_OFFMASK || c.dst_f32;
            const int r = c.store == CRFP_PROBE_ST_PS ? c.ps_r : 1, pad = c.store == CRFP_PROBE_ST_Q4 ? c.dst_pad[d] : 0;
            if (fdst) RUN(crfp::launch_q4_to_nchw(v.dst[d], c.dst[d], n, v.dst_ch[d], h * r, w * r, pad, s));
            else RUN(launch_q4_to_nchw(v.dst[d], c.dst[d], n, v.dst_ch[d], h * r, w * r, pad, s));
            if (c.dst_raw[d]) copy(c.dst_raw[d], v.dst[d], v.dst_bytes[d]);
        }
    }
    copy(status, P.status, 2 * (size_t)n * sizeof(unsigned));
    return rc;
}

}  // extern "C"
