// Test hook of the C-ABI (include/crfp_hip.h, crfp_gather_probe): ONE launch of the engines' own gather kernels (gather.hip, dcn_fused.inc) on
// caller-supplied NCHW fp32 tensors.  No sampling, blending, convolution or activation kernel of its own, and no kernel at all: the layouts come
// from launch_nchw_to_q4 / launch_offmask_nchw_to_q4 / launch_q4_to_nchw and pitched device copies, the weight images from pack_items over the
// plan items the engines build (add_mfma with ST_DCNFUSE rows, add_narrow with NE_OFFMASK3, the T_DCN8 / T_RAW weight items), and the launch
// goes through launch_flow_warp_q4 / launch_flow_warp_p4_dual_8_6 / launch_dcn_g8 / launch_dcn_fused / launch_dcn3 / launch_dcn3_fused with the
// arguments bound field for field as Runner::frame (engine.hip) binds them.  What differs is where the tensors live: in the caller's workspace,
// every one with a batch stride of its own (slack between the items), sampled tensors in padded planes behind a zeroed guard, destinations
// filled with 0xFF bytes.
// fp32 build, CRFP_GPROBE_DCN_FUSED: the offset feature must arrive as an SRC_S3 image, and the library's only producer of one is a conv's
// s3_dst -- one centre-tap identity conv (32 -> 32, no activation, no other destination) through launch_conv_mfma, as the S3 chain of
// conv_probe.hip.  Weight 1.0 has no low fp16 part and x0 + x1s * 2^-11 has 22 significant bits, so the conv's fp32 sum is that value exactly
// and the image holds x to the 22 bits of the fp16 pair (x itself where x has no more bits than that).
// Compiled twice (csrc/Makefile): crfp_gather_probe and crfp_gather_probe_bf16.
#include "engine_host.h"

namespace CRFP_NS {
namespace {

constexpr int kMaxN = 65535;

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

// One tensor of the launch: `packed` is what the library's conversion writes or reads (items back to back), `strided` what the kernel sees
// (item k at first() + k * stride elements; `lead` bytes in front of item 0).
struct Tensor {
    char *packed = nullptr, *strided = nullptr;
    size_t item = 0, stride = 0, lead = 0, esize = 0;   // item, stride, lead: bytes
    bool on = false;
    char* first() const { return strided + lead; }
    long long bs() const { return (long long)(stride / esize); }
    size_t strided_bytes(int n) const { return lead + (size_t)n * stride; }
};

enum { T_X = 0, T_X2, T_AUX, T_FLOW, T_OUT, T_OUT2, T_COUNT };

struct Probe {
    const crfp_gather_args* a = nullptr;
    int mode = 0, n = 0, h = 0, w = 0, nq = 0;
    Tensor t[T_COUNT];
    Item items[3];   // 0: the head (DCN_FUSED, DCN3_FUSED); 1: the identity conv that writes the S3 image (fp32 DCN_FUSED); 2: the DCN weights
    int count = 0;
    float* packed = nullptr;
    size_t packed_floats = 0;
    float* ident = nullptr;        // identity weights [32][32][3][3] and a zero bias [32]
    float* featq = nullptr;        // fp32 DCN_FUSED: the offset feature as fp32 Q4, the identity conv's source
    unsigned *status = nullptr, *status2 = nullptr;
    size_t bytes = 0;
};

constexpr size_t kIdentFloats = 32 * 32 * 9 + 32;
const float* ident_host() {
    static const float* const v = [] {
        float* p = new float[kIdentFloats]();
        for (int c = 0; c < 32; ++c) p[(c * 32 + c) * 9 + 4] = 1.0f;
        return p;
    }();
    return v;
}

bool dcn_mode(int m) { return m >= CRFP_GPROBE_DCN_G8; }

// validates the call, builds the plan items and lays the workspace out behind `base` (null: sizes only)
int prepare(Probe& P, const crfp_gather_args* a, char* base, bool need_ptrs) {
    if (!a) { set_error("gather_probe: null argument block"); return CRFP_E_BADARG; }
    if (a->mode < CRFP_GPROBE_WARP || a->mode > CRFP_GPROBE_DCN3_FUSED) { set_error("gather_probe: unknown mode %d", a->mode); return CRFP_E_BADARG; }
    const int mode = a->mode, n = a->n, h = a->h, w = a->w;
    if (n < 1 || n > kMaxN || h < 1 || w < 1) { set_error("gather_probe: bad geometry (n=%d h=%d w=%d)", n, h, w); return CRFP_E_BADARG; }
    // the hook's own limit, below the launchers' (launch_dcn_g8: 2^24 elements): the warps address 8 planes of 16-byte quads with 32-bit byte offsets
    if ((long long)(h + 1) * (w + 1) >= (1ll << 22)) { set_error("gather_probe: plane of %d x %d exceeds the hook's 2^22-element range", h, w); return CRFP_E_UNSUPPORTED; }
    if (mode == CRFP_GPROBE_WARP && a->c != 4 && a->c != 24 && a->c != 32) { set_error("gather_probe: a warp takes 4, 24 or 32 channels (c = %d)", a->c); return CRFP_E_BADARG; }
    // the engines' own condition for the fused launch (Runner::frame): SRC_S3 edges (fp32 build) and the split-fp16 DCN GEMM
    if (mode == CRFP_GPROBE_DCN_FUSED && ((!kActBf16 && !conv_s3_supported()) || !dcn_g8_use_f16())) {
        set_error("gather_probe: the fused DCN launch needs the default conv / DCN kernels (no CRFP_PRECISION override)");
        return CRFP_E_UNSUPPORTED;
    }
    if (mode == CRFP_GPROBE_DCN_G8 && !dcn_g8_use_f16()) { set_error("gather_probe: the engines' dcn_g8 runs on the split-fp16 image (no CRFP_PRECISION override)"); return CRFP_E_UNSUPPORTED; }
    const bool fused = mode == CRFP_GPROBE_DCN_FUSED || mode == CRFP_GPROBE_DCN3_FUSED;
    const bool dual = mode == CRFP_GPROBE_WARP_DUAL;
    const bool has_aux = dcn_mode(mode), has_flow = !dcn_mode(mode) || fused;
    if (need_ptrs) {
        if (!a->x || !a->out || !a->status || (dual && (!a->x2 || !a->out2)) || (has_aux && !a->aux) || (mode == CRFP_GPROBE_DCN_G8 && !a->mask) || (has_flow && !a->flow)) {
            set_error("gather_probe: null tensor");
            return CRFP_E_BADARG;
        }
        if (dcn_mode(mode) && (!a->weight || !a->bias)) { set_error("gather_probe: null weight or bias"); return CRFP_E_BADARG; }
        if (fused && (!a->head_w || !a->head_b)) { set_error("gather_probe: null head weight or bias"); return CRFP_E_BADARG; }
    }
    P.a = a; P.mode = mode; P.n = n; P.h = h; P.w = w;
    const int cx = mode == CRFP_GPROBE_WARP ? a->c : (mode >= CRFP_GPROBE_DCN3 ? 4 : 32);
    P.nq = cx / 4;
    const size_t px = (size_t)h * w, ppx = (size_t)(h + 1) * (w + 1);
    // slack between batch items: the zeroed guard a P4 plane needs in front of it (one pad row + one quad), and more -- different per tensor
    const size_t guard_q = (size_t)w + 2;
    int k = 0;
    auto lay = [&](Tensor& t, size_t quads, size_t qbytes, bool lead) {
        t.on = true;
        t.esize = qbytes / 4;
        t.item = quads * qbytes;
        t.stride = align_up(t.item, 256) + align_up(guard_q * qbytes, 256) + 256 * (size_t)(++k);
        t.lead = lead ? align_up(guard_q * qbytes, 256) : 0;
    };
    lay(P.t[T_X], (size_t)P.nq * ppx, kQuadBytes, true);
    if (dual) lay(P.t[T_X2], 6 * ppx, kQuadBytes, true);
    if (mode == CRFP_GPROBE_DCN_G8) lay(P.t[T_AUX], 54 * px, 16, false);
    else if (mode == CRFP_GPROBE_DCN_FUSED) lay(P.t[T_AUX], 8 * px, kQuadBytes, false);   // fp32: the SRC_S3 image, the same bytes
    else if (mode == CRFP_GPROBE_DCN3) lay(P.t[T_AUX], px, 16, false);
    else if (mode == CRFP_GPROBE_DCN3_FUSED) lay(P.t[T_AUX], px, kQuadBytes, false);
    if (has_flow) { lay(P.t[T_FLOW], px, 8, false); P.t[T_FLOW].esize = 4; }
    lay(P.t[T_OUT], (size_t)P.nq * px, kQuadBytes, false);
    if (dual) lay(P.t[T_OUT2], 6 * px, kQuadBytes, false);

    // plan items, as the clip engine's Model builds them
    const int FS = kActBf16 ? (int)SRC_Q4 : (int)SRC_S3;
    P.count = 3;
    for (Item& it : P.items) it = Item();
    if (mode == CRFP_GPROBE_DCN_FUSED) {
        add_mfma(P.items[0], "gather_probe:offset_mask_fused", 0, 1, 32, 216, {{FS, 32}}, ST_DCNFUSE, 0, CRFP_ACT_NONE, 1.0f);
        if (!kActBf16) add_mfma(P.items[1], "gather_probe:s3_identity", 2, -1, 32, 32, {{(int)SRC_Q4, 32}}, ST_Q4, 0, CRFP_ACT_NONE, 1.0f);
    } else if (mode == CRFP_GPROBE_DCN3_FUSED) {
        add_narrow(P.items[0], "gather_probe:dcn3.offset_mask", 0, 1, 4, 3, 0, {{(int)SRC_Q4, 4}}, CRFP_ACT_NONE, NE_OFFMASK3);
    }
    if (mode == CRFP_GPROBE_DCN_G8 || mode == CRFP_GPROBE_DCN_FUSED) {
        Item& dw = P.items[2];
        dw.type = T_DCN8; dw.name = "dcn_g8_weights"; dw.w1 = 3;
        dw.n_w = 2 * 36 * 2 * 32 * 4; dw.n_b = 32;
    } else if (mode >= CRFP_GPROBE_DCN3) {
        Item& d3 = P.items[2];
        d3.type = T_RAW; d3.name = "dcn3_weights"; d3.w1 = 3;
        d3.n_w = 4 * 4 * 9; d3.n_b = 4;
    }
    P.packed_floats = assign_offsets(P.items, P.count);

    Bump B{base};
    P.packed = (float*)B.take(P.packed_floats * sizeof(float));
    P.status = (unsigned*)B.take((size_t)n * sizeof(unsigned));
    P.status2 = (unsigned*)B.take((size_t)n * sizeof(unsigned));
    if (mode == CRFP_GPROBE_DCN_FUSED && !kActBf16) {
        P.ident = (float*)B.take(kIdentFloats * sizeof(float));
        P.featq = (float*)B.take((size_t)n * 8 * px * 16);
    }
    for (Tensor& t : P.t) {
        if (!t.on) continue;
        t.packed = B.take((size_t)n * t.item);
        t.strided = B.take(t.strided_bytes(n));
    }
    P.bytes = align_up(B.off, 256);
    return 0;
}

// which kernel the launch takes: the launchers' own rules (gather.hip, dcn_fused.inc)
int report_of(const Probe& P, crfp_gather_report* r) {
    memset(r, 0, sizeof(*r));
    r->out_stride = P.t[T_OUT].bs();
    r->out2_stride = P.t[T_OUT2].on ? P.t[T_OUT2].bs() : 0;
    switch (P.mode) {
        case CRFP_GPROBE_WARP: r->kernel = CRFP_GATHERK_WARP_P4; break;
        case CRFP_GPROBE_WARP_DUAL:
            r->split = flow_warp_dual_split(P.n);
            r->kernel = r->split ? CRFP_GATHERK_WARP_DUAL_SPLIT : CRFP_GATHERK_WARP_DUAL;
            break;
        case CRFP_GPROBE_DCN_G8: r->kernel = CRFP_GATHERK_DCN_G8_PIPE; break;
        case CRFP_GPROBE_DCN_FUSED: {
            const DcnFusedGrid g = dcn_fused_grid(P.n, P.h, P.w);
            if (g.cus <= 0) return CRFP_E_UNSUPPORTED;
            r->cus = g.cus; r->tiles = g.tiles; r->persistent = g.persistent;
            r->kernel = g.persistent ? CRFP_GATHERK_DCN_FUSED_PS : CRFP_GATHERK_DCN_FUSED;
            break;
        }
        case CRFP_GPROBE_DCN3: r->kernel = CRFP_GATHERK_DCN3; break;
        default: r->kernel = CRFP_GATHERK_DCN3_FUSED;
    }
    return 0;
}

}  // namespace
}  // namespace CRFP_NS

using namespace CRFP_NS;

extern "C" {

size_t CRFP_API(crfp_gather_probe_workspace_bytes)(const crfp_gather_args* args) {
    Probe P;
    return prepare(P, args, nullptr, false) ? 0 : P.bytes;
}

int CRFP_API(crfp_gather_probe_plan)(const crfp_gather_args* args, crfp_gather_report* report) {
    if (!report) { set_error("gather_probe_plan: null result pointer"); return CRFP_E_BADARG; }
    Probe P;
    const int rc = prepare(P, args, nullptr, false);
    return rc ? rc : report_of(P, report);
}

int CRFP_API(crfp_gather_probe)(const crfp_gather_args* args, crfp_gather_report* report, void* workspace, size_t workspace_bytes, void* stream) {
    if (!report) { set_error("gather_probe: null result pointer"); return CRFP_E_BADARG; }
    Probe P;
    int rc = prepare(P, args, (char*)workspace, true);
    if (rc) return rc;
    if (!workspace || workspace_bytes < P.bytes) { set_error("gather_probe: workspace too small"); return CRFP_E_WORKSPACE; }
    rc = report_of(P, report);
    if (rc) return rc;
    const crfp_gather_args& a = *args;
    const int mode = P.mode, n = P.n, h = P.h, w = P.w;
    hipStream_t s = (hipStream_t)stream;
    auto fill = [&](void* p, int byte, size_t bytes) {
        if (!rc && bytes && hipMemsetAsync(p, byte, bytes, s) != hipSuccess) { set_error("gather_probe: memset failed"); rc = 1; }
    };
    auto copy = [&](void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
        if (!rc && bytes && hipMemcpyAsync(dst, src, bytes, kind, s) != hipSuccess) { set_error("gather_probe: copy failed"); rc = 1; }
    };
    // items back to back <-> items at the tensor's own stride
    auto spread = [&](const Tensor& t, const void* src) {
        if (!rc && hipMemcpy2DAsync(t.first(), t.stride, src, t.item, t.item, n, hipMemcpyDeviceToDevice, s) != hipSuccess) { set_error("gather_probe: copy failed"); rc = 1; }
    };
    auto gather = [&](const Tensor& t) {
        if (!rc && hipMemcpy2DAsync(t.packed, t.item, t.first(), t.stride, t.item, n, hipMemcpyDeviceToDevice, s) != hipSuccess) { set_error("gather_probe: copy failed"); rc = 1; }
    };
    fill(P.status, 0, (size_t)n * sizeof(unsigned));
    fill(P.status2, 0, (size_t)n * sizeof(unsigned));
    // weights: the engines' pack loop over this call's items
    if (P.ident) copy(P.ident, ident_host(), kIdentFloats * sizeof(float), hipMemcpyHostToDevice);
    const bool d3 = mode == CRFP_GPROBE_DCN3_FUSED;
    const int split = d3 ? 2 : 144;   // a head's offset rows, then its mask rows: two convs of the reference, one [216 | 3]-row tensor here
    const float* params[8] = {a.head_w, a.head_b, a.head_w ? a.head_w + (size_t)split * (d3 ? 4 : 32) * 9 : nullptr, a.head_b ? a.head_b + split : nullptr,
                              P.ident, P.ident ? P.ident + 32 * 32 * 9 : nullptr, a.weight, a.bias};
    RUN(pack_items(P.items, P.count, params, [&](int) { return split; }, P.packed, s));
    // tensors in: sampled tensors in padded planes behind zeros, everything at its own stride, destinations poisoned
    auto p4_in = [&](const Tensor& t, const float* src, int c) {
        fill(t.packed, 0, (size_t)n * t.item);
        fill(t.strided, 0, t.strided_bytes(n));
        RUN(launch_nchw_to_q4(src, (float*)t.packed, n, c, h, w, 1, s));
        spread(t, t.packed);
    };
    p4_in(P.t[T_X], a.x, 4 * P.nq);
    if (P.t[T_X2].on) p4_in(P.t[T_X2], a.x2, 24);
    const Tensor& aux = P.t[T_AUX];
    if (aux.on) fill(aux.strided, 0, aux.strided_bytes(n));
    if (mode == CRFP_GPROBE_DCN_G8) {
        RUN(crfp::launch_offmask_nchw_to_q4(a.aux, a.mask, (float*)aux.packed, n, 144, 72, h, w, s));
        spread(aux, aux.packed);
    } else if (mode == CRFP_GPROBE_DCN3) {
        RUN(crfp::launch_nchw_to_q4(a.aux, (float*)aux.packed, n, 3, h, w, 0, s, nullptr, 0));
        spread(aux, aux.packed);
    } else if (mode == CRFP_GPROBE_DCN3_FUSED || (mode == CRFP_GPROBE_DCN_FUSED && kActBf16)) {
        RUN(launch_nchw_to_q4(a.aux, (float*)aux.packed, n, mode == CRFP_GPROBE_DCN3_FUSED ? 4 : 32, h, w, 0, s));
        spread(aux, aux.packed);
    } else if (mode == CRFP_GPROBE_DCN_FUSED) {
        RUN(launch_nchw_to_q4(a.aux, P.featq, n, 32, h, w, 0, s));
        if (!rc) {
            ConvArgs p = bind_conv(P.items[1], P.packed, n, h, w, {{P.featq, 8LL * h * w * 4, 0}}, {}, P.status2);
            p.ovf_div = 1; p.ovf_add = 0;
            p.s3_dst = (float*)aux.first(); p.s3_bstride = aux.bs();
            rc = launch_conv_mfma(p, "gather_probe:s3_identity", s);
        }
    }
    const Tensor& fl = P.t[T_FLOW];
    if (fl.on) { fill(fl.strided, 0, fl.strided_bytes(n)); spread(fl, a.flow); }
    const Tensor &X = P.t[T_X], &O = P.t[T_OUT];
    fill(O.strided, 0xFF, O.strided_bytes(n));
    if (P.t[T_OUT2].on) fill(P.t[T_OUT2].strided, 0xFF, P.t[T_OUT2].strided_bytes(n));
    if (rc) return rc;
    // the launch, bound as Runner::frame binds it
    const Item& dw = P.items[2];
    switch (mode) {
        case CRFP_GPROBE_WARP:
            rc = launch_flow_warp_q4((const float*)X.first(), X.bs(), (const float*)fl.first(), fl.bs(), (float*)O.first(), O.bs(), n, P.nq, h, w, 0, 1, s);
            break;
        case CRFP_GPROBE_WARP_DUAL: {
            WarpDualStrides wb;
            wb.xa = X.bs(); wb.xb = P.t[T_X2].bs(); wb.flow = fl.bs(); wb.outa = O.bs(); wb.outb = P.t[T_OUT2].bs();
            rc = launch_flow_warp_p4_dual_8_6((const float*)X.first(), (const float*)P.t[T_X2].first(), (const float*)fl.first(), (float*)O.first(),
                                              (float*)P.t[T_OUT2].first(), h, w, s, n, wb);
            break;
        }
        case CRFP_GPROBE_DCN_G8:
            rc = launch_dcn_g8((const float*)X.first(), X.bs(), (const float*)aux.first(), aux.bs(), P.packed + dw.off_w + 36 * 2 * 32 * 4, P.packed + dw.off_b,
                               (float*)O.first(), O.bs(), n, h, w, s, true, P.status, 1);
            break;
        case CRFP_GPROBE_DCN_FUSED: {
            const Item& om = P.items[0];
            DcnFuseArgs fa;
            memset(&fa, 0, sizeof(fa));
            fa.feat = (const float*)aux.first(); fa.feat_b = aux.bs(); fa.flow = (const float*)fl.first(); fa.flow_b = fl.bs();
            fa.wconv = (const char*)(P.packed + om.off_s) + conv_split16_offset_bytes(om.c); fa.bconv = P.packed + om.off_b;
            fa.x = (const float*)X.first(); fa.xb = X.bs();
            fa.wdcn = P.packed + dw.off_w + 36 * 2 * 32 * 4; fa.bdcn = P.packed + dw.off_b;
            fa.out = (float*)O.first(); fa.ob = O.bs(); fa.N = n; fa.H = h; fa.W = w; fa.ovf = P.status; fa.ovf_div = 1;
            rc = launch_dcn_fused(fa, s);
            break;
        }
        case CRFP_GPROBE_DCN3:
            rc = launch_dcn3((const float*)X.first(), X.bs(), (const float*)aux.first(), aux.bs(), P.packed + dw.off_w, P.packed + dw.off_b, (float*)O.first(), O.bs(),
                             n, h, w, s);
            break;
        default: {
            const Item& om = P.items[0];
            rc = launch_dcn3_fused((const float*)X.first(), X.bs(), (const float*)aux.first(), aux.bs(), (const float*)fl.first(), P.packed + om.off_w,
                                   P.packed + om.off_b, P.packed + dw.off_w, P.packed + dw.off_b, (float*)O.first(), O.bs(), n, h, w, s, fl.bs());
        }
    }
    // tensors out
    auto out = [&](const Tensor& t, float* dst, void* raw, int c) {
        gather(t);
        RUN(launch_q4_to_nchw((const float*)t.packed, dst, n, c, h, w, 0, s));
        if (raw) copy(raw, t.strided, t.strided_bytes(n), hipMemcpyDeviceToDevice);
    };
    out(O, a.out, a.out_raw, 4 * P.nq);
    if (P.t[T_OUT2].on) out(P.t[T_OUT2], a.out2, a.out2_raw, 24);
    copy(a.status, P.status, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToDevice);
    return rc;
}

}  // extern "C"
