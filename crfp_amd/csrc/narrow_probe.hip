// Test hook of the C-ABI (include/crfp_hip.h, crfp_narrow_probe): ONE launch of the engines' own 8x narrow conv kernels (conv_narrow.hip) on
// caller-supplied tensors.  No kernel of its own: the plans come from add_narrow (engine_host.h), the weight images from pack_items
// (launch_narrow_pack), the launch goes through launch_narrow / launch_narrow_pair / launch_narrow_chain with the NarrowArgs bound field for field
// as Runner::narrow / narrow_pair / narrow_chain (engine.hip) and narrow (engine_rt.hip) bind them, the gate flags come from launch_mask_gate.
// What differs is where the tensors live: in the caller's workspace, converted from and to NCHW fp32 by this namespace's launch_nchw_to_q4 /
// launch_q4_to_nchw, so that the storage type is the build's.  Compiled twice (csrc/Makefile): crfp_narrow_probe and crfp_narrow_probe_bf16.
#include "engine_host.h"

namespace CRFP_NS {
namespace {

constexpr int kMaxN = 65535;
constexpr int kWindowFill = 0x3F;   // bytes of the planes around a window source: 0.747 as fp32, 0.746 as bf16 -- never zero

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

struct Stage {   // one stencil of a call: its plan item, its device tensors, the launch-time plan
    const crfp_narrow_stencil* c = nullptr;
    Item it;
    int first_own = 0;                 // index in the plan's source table of the first source this stencil brings itself
    char* src[3] = {};                 // buffers of its own Q4 sources (a window source: lead included)
    size_t src_bytes[3] = {}, src_lead[3] = {};
    float* resid = nullptr;
    NarrowArgs plan;
};

struct Probe {
    int mode = 0, res = 0, n = 0, h = 0, w = 0, count = 0;
    Stage st[3];
    float* packed = nullptr;
    size_t packed_floats = 0;
    unsigned* status = nullptr;
    uint8_t* gate = nullptr;
    long long gate_b = 0;
    char* dst = nullptr;               // the last stencil's destination (NE_LAST: the caller's tensor, no buffer here)
    size_t dst_bytes = 0;
    char* dst2 = nullptr;
    size_t dst2_bytes = 0;
    size_t bytes = 0;
};

const char* const kWho[3] = {"a", "b", "c"};

// how many sources a stencil may bring itself: a has all of its own, a pair's b none, a chain's b none and its c at most one global quad
int own_limit(int mode, int k) { return k == 0 ? 3 : (mode == CRFP_NPROBE_CHAIN && k == 2 ? 1 : 0); }

int check_stencil(const Probe& P, const crfp_narrow_stencil& c, int k, bool need_ptrs) {
    const char* who = kWho[k];
    const bool last = k == P.count - 1;
    const int h = P.h, w = P.w;
    if (c.nsrc < (k == 0 ? 1 : 0) || c.nsrc > 3) { set_error("narrow_probe %s: %d sources", who, c.nsrc); return CRFP_E_BADARG; }
    int quads = 0;
    for (int i = 0; i < c.nsrc; ++i) {
        const int kind = c.src_kind[i], nch = c.src_nch[i];
        if (kind != CRFP_PROBE_SRC_Q4 && kind != CRFP_PROBE_SRC_FLOW2) { set_error("narrow_probe %s: source %d of unknown kind %d", who, i, kind); return CRFP_E_BADARG; }
        if (nch < 1 || nch > 4 || (kind == CRFP_PROBE_SRC_FLOW2 && nch != 2)) { set_error("narrow_probe %s: source %d has %d channels (Q4: 1 .. 4, flow: 2)", who, i, nch); return CRFP_E_BADARG; }
        if (need_ptrs && !c.src[i]) { set_error("narrow_probe %s: null source %d", who, i); return CRFP_E_BADARG; }
        ++quads;
    }
    if (k > 0 && c.nsrc > own_limit(P.mode, k)) {
        if (P.mode == CRFP_NPROBE_PAIR) set_error("narrow_probe b: a pair's second stencil reads one quad, the first stencil's output (%d more given)", c.nsrc);
        else set_error("narrow_probe %s: this stencil of a chain brings at most %d global quad(s) of its own (%d given)", who, own_limit(P.mode, k), c.nsrc);
        return CRFP_E_BADARG;
    }
    if (quads + (k > 0 ? 1 : 0) > 3) { set_error("narrow_probe %s: more than 3 input quads", who); return CRFP_E_BADARG; }
    if (c.cout < 1 || c.cout > 4) { set_error("narrow_probe %s: cout %d (1 .. 4)", who, c.cout); return CRFP_E_BADARG; }
    if (c.act != CRFP_ACT_NONE && c.act != CRFP_ACT_RELU && c.act != CRFP_ACT_LRELU01) { set_error("narrow_probe %s: activation %d (none, relu, lrelu 0.1)", who, c.act); return CRFP_E_BADARG; }
    if (c.epi < NE_PLAIN || c.epi > NE_OFFMASK3) { set_error("narrow_probe %s: unknown epilogue %d", who, c.epi); return CRFP_E_BADARG; }
    if (need_ptrs && (!c.weight || !c.bias)) { set_error("narrow_probe %s: null weight or bias", who); return CRFP_E_BADARG; }
    if (c.cout_split > 0 && (c.cout_split >= c.cout || (need_ptrs && (!c.weight2 || !c.bias2)))) {
        set_error("narrow_probe %s: cout_split %d needs 0 < cout_split < cout and weight2 / bias2", who, c.cout_split);
        return CRFP_E_BADARG;
    }
    if (c.src_pad < 0 || c.dst_pad < 0 || (c.src_pad && (c.nsrc < 1 || c.src_kind[0] != CRFP_PROBE_SRC_Q4))) {
        set_error("narrow_probe %s: pads are >= 0 and only a Q4 source 0 comes in padded planes (src_pad %d, dst_pad %d)", who, c.src_pad, c.dst_pad);
        return CRFP_E_BADARG;
    }
    if (P.count > 1 && (c.src_pad || c.dst_pad)) { set_error("narrow_probe %s: the engines bind pairs and chains with unpadded tensors", who); return CRFP_E_BADARG; }
    if (c.dst_pad && c.epi != NE_PLAIN && c.epi != NE_BLEND) { set_error("narrow_probe %s: only a Q4 destination comes in padded planes", who); return CRFP_E_BADARG; }
    if (!last) {
        if (c.dst2_on || c.gate_h >= 0) { set_error("narrow_probe %s: only the last stencil of a launch has a second destination or a gate", who); return CRFP_E_BADARG; }
        return 0;
    }
    if (c.gate_h > 3) { set_error("narrow_probe %s: gate_h %d (0 .. 3, < 0: dense)", who, c.gate_h); return CRFP_E_BADARG; }
    if (c.gate_h >= 0) {
        if (P.count > 1) { set_error("narrow_probe %s: no mask-gated form of a pair or chain", who); return CRFP_E_UNSUPPORTED; }
        if (c.dst2_on) { set_error("narrow_probe %s: no mask-gated form with a second destination", who); return CRFP_E_UNSUPPORTED; }
        if (w & 3) { set_error("narrow_probe %s: launch_mask_gate reads the mask four bytes at a time (w = %d)", who, w); return CRFP_E_BADARG; }
    }
    if ((c.epi == NE_BLEND || c.gate_h >= 0) && need_ptrs && !c.mask) { set_error("narrow_probe %s: null mask", who); return CRFP_E_BADARG; }
    if (c.epi == NE_OFFMASK3 && need_ptrs && !c.flow) { set_error("narrow_probe %s: null flow", who); return CRFP_E_BADARG; }
    if (c.epi == NE_LAST && ((h & 7) || (w & 7) || (need_ptrs && !c.base_lr))) { set_error("narrow_probe %s: the output head takes h, w multiples of 8 and base_lr (h=%d w=%d)", who, h, w); return CRFP_E_BADARG; }
    if (need_ptrs && (!c.dst || (c.dst2_on && !c.dst2))) { set_error("narrow_probe %s: null destination", who); return CRFP_E_BADARG; }
    return 0;
}

// validates the call, builds the plan items and lays the workspace out behind `base` (null: sizes only)
int prepare(Probe& P, int mode, const crfp_narrow_stencil* a, const crfp_narrow_stencil* b, const crfp_narrow_stencil* c, int res, int n, int h, int w,
            char* base, bool need_ptrs) {
    if (mode < CRFP_NPROBE_SINGLE || mode > CRFP_NPROBE_CHAIN) { set_error("narrow_probe: unknown mode %d", mode); return CRFP_E_BADARG; }
    if (!a || (mode != CRFP_NPROBE_SINGLE && !b) || (mode == CRFP_NPROBE_CHAIN && !c)) { set_error("narrow_probe: null stencil descriptor"); return CRFP_E_BADARG; }
    if (n < 1 || n > kMaxN || h < 1 || w < 1 || (long long)h * w > (1LL << 24)) { set_error("narrow_probe: bad geometry (n=%d h=%d w=%d)", n, h, w); return CRFP_E_BADARG; }
    P.mode = mode; P.res = res != 0; P.n = n; P.h = h; P.w = w;
    P.count = mode + 1;
    P.st[0].c = a; P.st[1].c = b; P.st[2].c = c;
    for (int k = 0; k < P.count; ++k) {
        const int rc = check_stencil(P, *P.st[k].c, k, need_ptrs);
        if (rc) return rc;
    }
    Bump B{base};
    Item items[3];
    for (int k = 0; k < P.count; ++k) {
        Stage& v = P.st[k];
        const crfp_narrow_stencil& d = *v.c;
        std::vector<SrcSpec> specs;
        if (k > 0) specs.push_back({(int)SRC_Q4, 4});   // the quad the stencil before it leaves in LDS
        v.first_own = (int)specs.size();
        int cin = 4 * v.first_own;
        for (int i = 0; i < d.nsrc; ++i) { specs.push_back({d.src_kind[i], d.src_nch[i]}); cin += d.src_nch[i]; }
        static const char* const names[3] = {"narrow_probe:a", "narrow_probe:b", "narrow_probe:c"};
        add_narrow(items[k], names[k], 2 * k, d.cout_split > 0 ? 2 * k + 1 : -1, cin, d.cout, d.y_only, specs, d.act, d.epi);
        items[k].nw.post_scale = d.post_scale;
    }
    P.packed_floats = assign_offsets(items, P.count);
    P.packed = (float*)B.take(P.packed_floats * sizeof(float));
    P.status = (unsigned*)B.take((size_t)n * sizeof(unsigned));
    const size_t px = (size_t)h * w;
    for (int k = 0; k < P.count; ++k) {
        Stage& v = P.st[k];
        const crfp_narrow_stencil& d = *v.c;
        v.it = items[k];
        for (int i = 0; i < d.nsrc; ++i) {
            if (d.src_kind[i] != CRFP_PROBE_SRC_Q4) continue;
            const size_t pad = i == 0 ? d.src_pad : 0;
            // a window source (pad > 1) sits two rows and two columns inside its wider planes: what lies above and left of it is not zero either
            v.src_lead[i] = pad > 1 ? align_up((2 * (w + pad) + 2) * kQuadBytes, 256) : 0;
            v.src_bytes[i] = v.src_lead[i] + (size_t)n * (h + pad) * (w + pad) * kQuadBytes;
            v.src[i] = B.take(v.src_bytes[i]);
        }
        if (d.residual) v.resid = (float*)B.take((size_t)n * px * kQuadBytes);
    }
    const crfp_narrow_stencil& L = *P.st[P.count - 1].c;
    if (L.gate_h >= 0) {
        P.gate_b = (long long)align_up((size_t)4 * ((w + 63) / 64) * ((h + 15) / 16), 256);
        P.gate = (uint8_t*)B.take((size_t)n * P.gate_b);
    }
    if (L.epi == NE_PLAIN || L.epi == NE_BLEND) P.dst_bytes = (size_t)n * (h + L.dst_pad) * (w + L.dst_pad) * kQuadBytes;
    else if (L.epi == NE_OFFMASK3) P.dst_bytes = (size_t)n * px * 16;
    if (P.dst_bytes) P.dst = B.take(P.dst_bytes);
    if (L.dst2_on) { P.dst2_bytes = (size_t)n * (h + 1) * (w + 1) * kQuadBytes; P.dst2 = B.take(P.dst2_bytes); }
    P.bytes = align_up(B.off, 256);
    return 0;
}

// the launch-time plans, field for field as the engines' binders set them (Runner::narrow / narrow_pair / narrow_chain)
void bind(Probe& P, const float* packed) {
    const int n = P.n, h = P.h, w = P.w;
    const long long px = (long long)h * w;
    for (int k = 0; k < P.count; ++k) {
        Stage& v = P.st[k];
        const crfp_narrow_stencil& d = *v.c;
        const bool last = k == P.count - 1;
        NarrowArgs& a = v.plan;
        a = v.it.nw;
        for (int i = 0; i < d.nsrc; ++i) {
            ConvSrc& s = a.src[v.first_own + i];
            const long long pad = i == 0 ? d.src_pad : 0;
            if (d.src_kind[i] == CRFP_PROBE_SRC_Q4) { s.p = (const float*)(v.src[i] + v.src_lead[i]); s.bstride = (h + pad) * (w + pad) * 4; }
            else { s.p = d.src[i]; s.bstride = px * 2; }
            s.pad = 0;
        }
        a.src[0].pad = d.src_pad;
        a.dst_pad = d.dst_pad;
        a.N = n; a.H = h; a.W = w;
        a.wpk = packed + v.it.off_w;
        a.bpk = packed + v.it.off_b;
        a.resid = v.resid; a.resid_bstride = px * 4;
        if (!last) continue;
        if (d.epi == NE_LAST) { a.dst = d.dst; a.dst_bstride = (d.y_only ? 1 : 3) * px; }
        else { a.dst = (float*)P.dst; a.dst_bstride = d.epi == NE_OFFMASK3 ? px * 4 : (long long)(h + d.dst_pad) * (w + d.dst_pad) * 4; }
        a.flow = d.flow; a.flow_bstride = px * 2;
        a.base = nullptr; a.base_lr = d.base_lr; a.base_bstride = 3LL * (h >> 3) * (w >> 3);
        a.mask = d.mask; a.mask_bstride = px;
        a.ovf = P.status; a.ovf_div = 1; a.ovf_add = 0;   // every batch item its own status word
        a.dst2 = (float*)P.dst2; a.dst2_bstride = (long long)(h + 1) * (w + 1) * 4;
        if (d.gate_h >= 0) { a.gate = P.gate; a.gate_bstride = P.gate_b; a.gate_h = d.gate_h; }
    }
}

// which kernel, with which template arguments, on how many workgroups: the launchers' own sizing functions (conv_narrow.hip)
void report_of(const Probe& P, crfp_narrow_report* r) {
    memset(r, 0, sizeof(*r));
    const NarrowArgs& a = P.st[0].plan;
    const NarrowArgs& l = P.st[P.count - 1].plan;
    NarrowGrid g;
    if (P.mode == CRFP_NPROBE_SINGLE) g = narrow_grid(a);
    else if (P.mode == CRFP_NPROBE_PAIR) g = narrow_pair_grid(a);
    else g = narrow_chain_grid(a);
    r->kernel = g.kernel; r->tiles = g.tiles; r->workgroups = g.workgroups;
    r->kq = a.kq;
    r->epi = l.epi;
    r->gate = g.kernel == NK_NARROW && a.gate != nullptr;
    r->st2 = l.dst2 != nullptr && !r->gate;
    r->kqg = P.mode == CRFP_NPROBE_CHAIN ? l.kq - 1 : 0;
    r->res = P.mode == CRFP_NPROBE_CHAIN ? P.res : 0;
}

}  // namespace
}  // namespace CRFP_NS

using namespace CRFP_NS;

extern "C" {

size_t CRFP_API(crfp_narrow_probe_workspace_bytes)(int mode, const crfp_narrow_stencil* a, const crfp_narrow_stencil* b, const crfp_narrow_stencil* c,
                                                   int res, int n, int h, int w) {
    Probe P;
    return prepare(P, mode, a, b, c, res, n, h, w, nullptr, false) ? 0 : P.bytes;
}

int CRFP_API(crfp_narrow_probe_plan)(int mode, const crfp_narrow_stencil* a, const crfp_narrow_stencil* b, const crfp_narrow_stencil* c, int res, int n,
                                     int h, int w, crfp_narrow_report* report) {
    if (!report) { set_error("narrow_probe_plan: null result pointer"); return CRFP_E_BADARG; }
    Probe P;
    const int rc = prepare(P, mode, a, b, c, res, n, h, w, nullptr, false);
    if (rc) return rc;
    bind(P, reinterpret_cast<const float*>(256));
    // sizes only: no buffer exists, but the rule asks whether a gate and a second destination are there
    NarrowArgs& l = P.st[P.count - 1].plan;
    const crfp_narrow_stencil& L = *P.st[P.count - 1].c;
    if (L.gate_h >= 0) l.gate = reinterpret_cast<const uint8_t*>(256);
    if (L.dst2_on) l.dst2 = reinterpret_cast<float*>(256);
    report_of(P, report);
    return 0;
}

int CRFP_API(crfp_narrow_probe)(int mode, const crfp_narrow_stencil* a, const crfp_narrow_stencil* b, const crfp_narrow_stencil* c, int res, int n, int h,
                                int w, const unsigned* status_in, unsigned* status_out, crfp_narrow_report* report, void* workspace,
                                size_t workspace_bytes, void* stream) {
    if (!status_out || !report) { set_error("narrow_probe: null status or report pointer"); return CRFP_E_BADARG; }
    Probe P;
    int rc = prepare(P, mode, a, b, c, res, n, h, w, (char*)workspace, true);
    if (rc) return rc;
    if (!workspace || workspace_bytes < P.bytes) { set_error("narrow_probe: workspace too small"); return CRFP_E_WORKSPACE; }
    hipStream_t s = (hipStream_t)stream;
    auto fill = [&](void* p, int byte, size_t bytes) {
        if (!rc && bytes && hipMemsetAsync(p, byte, bytes, s) != hipSuccess) { set_error("narrow_probe: memset failed"); rc = 1; }
    };
    auto copy = [&](void* dst, const void* src, size_t bytes) {
        if (!rc && bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) { set_error("narrow_probe: copy failed"); rc = 1; }
    };
    if (status_in) copy(P.status, status_in, (size_t)n * sizeof(unsigned));
    else fill(P.status, 0, (size_t)n * sizeof(unsigned));
    // weights: the engines' pack loop over this call's items
    const float* params[12] = {};
    Item items[3];
    for (int k = 0; k < P.count; ++k) {
        const crfp_narrow_stencil& d = *P.st[k].c;
        params[4 * k] = d.weight; params[4 * k + 1] = d.bias; params[4 * k + 2] = d.weight2; params[4 * k + 3] = d.bias2;
        items[k] = P.st[k].it;
    }
    RUN(pack_items(items, P.count, params, [&](int ci) { return P.st[ci / 2].c->cout_split; }, P.packed, s));
    // tensors in: sources and residuals in the storage type, destinations poisoned
    const crfp_narrow_stencil& L = *P.st[P.count - 1].c;
    for (int k = 0; k < P.count; ++k) {
        Stage& v = P.st[k];
        const crfp_narrow_stencil& d = *v.c;
        for (int i = 0; i < d.nsrc; ++i) {
            if (d.src_kind[i] != CRFP_PROBE_SRC_Q4) continue;
            const int pad = i == 0 ? d.src_pad : 0;
            if (pad) fill(v.src[i], pad > 1 ? kWindowFill : 0, v.src_bytes[i]);
            RUN(launch_nchw_to_q4(d.src[i], (float*)(v.src[i] + v.src_lead[i]), n, d.src_nch[i], h, w, pad, s));
        }
        if (d.residual) RUN(launch_nchw_to_q4(d.residual, v.resid, n, 4, h, w, 0, s));
    }
    const size_t last_bytes = (size_t)n * (L.y_only ? 1 : 3) * h * w * sizeof(float);
    if (L.epi == NE_LAST) fill(L.dst, 0xFF, last_bytes);
    fill(P.dst, 0xFF, P.dst_bytes);
    fill(P.dst2, 0xFF, P.dst2_bytes);
    if (P.gate) {
        fill(P.gate, 0, (size_t)n * P.gate_b);
        RUN(launch_mask_gate(L.mask, (long long)h * w, P.gate, P.gate_b, n, h, w, s));
    }
    if (rc) return rc;
    bind(P, P.packed);
    report_of(P, report);
    switch (mode) {
        case CRFP_NPROBE_PAIR: rc = launch_narrow_pair(P.st[0].plan, P.st[1].plan, "narrow_probe:pair", s); break;
        case CRFP_NPROBE_CHAIN: rc = launch_narrow_chain(P.st[0].plan, P.st[1].plan, P.st[2].plan, P.res != 0, "narrow_probe:chain", s); break;
        default: rc = launch_narrow(P.st[0].plan, "narrow_probe:a", s);
    }
    // tensors out
    if (L.epi == NE_PLAIN || L.epi == NE_BLEND) RUN(launch_q4_to_nchw((const float*)P.dst, L.dst, n, 4, h, w, L.dst_pad, s));
    else if (L.epi == NE_OFFMASK3) RUN(crfp::launch_q4_to_nchw((const float*)P.dst, L.dst, n, 4, h, w, 0, s));
    if (L.dst_raw) copy(L.dst_raw, P.dst, P.dst_bytes);
    if (P.dst2) {
        RUN(launch_q4_to_nchw((const float*)P.dst2, L.dst2, n, 4, h, w, 1, s));
        if (L.dst2_raw) copy(L.dst2_raw, P.dst2, P.dst2_bytes);
    }
    copy(status_out, P.status, (size_t)n * sizeof(unsigned));
    return rc;
}

}  // extern "C"
