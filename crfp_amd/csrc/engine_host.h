// Host core shared by the clip engine (engine.hip, fp32 and bf16 builds) and the regional engine (engine_rt.hip): packed-weight items and
// their plan builders, the packed-buffer offsets and the pack loop, the per-thread stream tables, and the binding of a launch's tensors into
// a ConvArgs.  Host code only.  Each engine keeps what is its own: its conv table and channel rules, its item list, its Layout, its
// schedule, and the slot type (streams + event pool) its tables hold.
#pragma once
#include "crfp_common.h"

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

namespace CRFP_NS {

#define RUN(expr) do { if (!rc) rc = (expr); } while (0)

struct ConvDef { const char* stem; int cout, cin; };

// ------------------------------------------------------------------ packed items
enum ItemType { T_MFMA = 0, T_NARROW = 1, T_DCN8 = 2, T_RAW = 3 };
struct Item {
    int type = T_MFMA;
    ConvArgs c;
    NarrowArgs nw;
    int w1 = -1, w2 = -1;
    size_t off_w = 0, off_b = 0, n_w = 0, n_b = 0;  // float offsets / counts inside the packed buffer
    size_t off_s = 0, n_s = 0;                       // split-bf16 weight image (T_MFMA only), in floats
    const char* name = "";
};

struct SrcSpec { int kind, nch; };

// the source table of a plan; returns its K in quads.  A SRC_ZERO source stands for weight columns that are never read (0 * w == 0): it
// takes K but no input channels
template <class Args>
static int plan_sources(Args& a, const std::vector<SrcSpec>& srcs, bool pad_k16) {
    int kq = 0, cbase = 0;
    for (auto& s : srcs) {
        ConvSrc& d = a.src[a.nsrc++];
        d.kind = s.kind;
        d.nch = s.nch;
        d.nq = src_quads(s.kind, s.nch);
        d.cbase = cbase;
        if (s.kind != SRC_ZERO) cbase += s.nch;
        kq += d.nq;
    }
    if (pad_k16 && (kq & 3)) {  // K is consumed in chunks of 4 quads (16 channels) by the split-bf16 main loop
        ConvSrc& d = a.src[a.nsrc++];
        d.kind = SRC_ZERO;
        d.nq = 4 - (kq & 3);
        d.nch = d.nq;
        d.cbase = cbase;
        kq += d.nq;
    }
    return kq;
}

// cin_total / cout: the engine's own channel rules (cout: of both convs of a paired item)
static ConvArgs make_mfma(int cin_total, int cout, const std::vector<SrcSpec>& srcs, int store, int ps_r, int act, float post_scale) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.kq = plan_sources(a, srcs, true);
    a.cin_total = cin_total;
    a.cout = cout;
    a.store = store;
    a.ps_r = ps_r;
    a.act = act;
    a.post_scale = post_scale;
    a.ctiles = (conv_packed_rows(a.cout, store, ps_r) + 31) / 32;
    return a;
}

static NarrowArgs make_narrow(int cin_total, int cout, int y_only, const std::vector<SrcSpec>& srcs, int act, int epi) {
    NarrowArgs a;
    memset(&a, 0, sizeof(a));
    a.kq = plan_sources(a, srcs, false);
    a.cin_total = cin_total;
    a.cout = cout;
    a.act = act;
    a.epi = epi;
    a.y_only = y_only;
    a.post_scale = 1.0f;
    return a;
}

// ci / ci2: the item's conv(s) in the engine's conv table
static void add_mfma(Item& it, const char* name, int ci, int ci2, int cin_total, int cout, const std::vector<SrcSpec>& srcs, int store, int ps_r,
                     int act, float post_scale) {
    it.type = T_MFMA;
    it.name = name;
    it.w1 = ci;
    it.w2 = ci2;
    it.c = make_mfma(cin_total, cout, srcs, store, ps_r, act, post_scale);
    it.n_w = conv_packed_weight_floats(it.c);
    it.n_b = (size_t)it.c.ctiles * 32;
    it.n_s = conv_split_weight_bytes(it.c) / sizeof(float);
}
static void add_narrow(Item& it, const char* name, int ci, int ci2, int cin_total, int cout, int y_only, const std::vector<SrcSpec>& srcs, int act,
                       int epi) {
    it.type = T_NARROW;
    it.name = name;
    it.w1 = ci;
    it.w2 = ci2;
    it.nw = make_narrow(cin_total, cout, y_only, srcs, act, epi);
    it.n_w = narrow_packed_weight_floats(it.nw);
    it.n_b = 4;
}

// places every item's weights, bias and split image in the packed buffer (64-float alignment); returns the buffer's size in floats
static size_t assign_offsets(Item* items, int count) {
    size_t cur = 0;
    for (int i = 0; i < count; ++i) {
        Item& it = items[i];
        if (it.w1 < 0) continue;
        it.off_w = cur;
        cur += (it.n_w + 63) / 64 * 64;
        it.off_b = cur;
        cur += (it.n_b + 63) / 64 * 64;
        it.off_s = cur;
        cur += (it.n_s + 63) / 64 * 64;
    }
    return cur;
}

#ifdef CRFP_ACT_BF16
int round_bf16_copy(const float* src, float* dst, int n, hipStream_t s);   // engine.hip: raw weights become bf16 values on their way in
#endif

// params: (weight, bias) device pointers in the order of the engine's conv table; split_of(ci): cout of conv ci, where a paired item's
// second conv begins
template <class SplitOf>
static int pack_items(const Item* items, int count, const float* const* params, SplitOf split_of, float* pk, hipStream_t s) {
    for (int i = 0; i < count; ++i) {
        const Item& it = items[i];
        if (it.w1 < 0) continue;
        const float* w = params[2 * it.w1];
        const float* b = params[2 * it.w1 + 1];
        const float* w2 = it.w2 >= 0 ? params[2 * it.w2] : nullptr;
        const float* b2 = it.w2 >= 0 ? params[2 * it.w2 + 1] : nullptr;
        const int split = split_of(it.w1);
        int rc = 0;
        switch (it.type) {
            case T_MFMA:
                rc = launch_conv_pack(it.c, w, b, w2, b2, split, pk + it.off_w, pk + it.off_b, s);
                if (!rc) rc = launch_conv_pack_split(it.c, w, w2, split, pk + it.off_s, s);
                break;
            case T_NARROW: rc = launch_narrow_pack(it.nw, w, b, w2, b2, split, pk + it.off_w, pk + it.off_b, s); break;
            case T_DCN8:
                if (!kActBf16) rc = launch_dcn_g8_pack(w, pk + it.off_w, s, false);   // fp32 MFMA image (strict mode, fp32 build)
                if (!rc) rc = launch_dcn_g8_pack(w, pk + it.off_w + 36 * 2 * 32 * 4, s, true);
                if (!rc && hipMemcpyAsync(pk + it.off_b, b, 32 * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) rc = 1;
                break;
            default:
#ifdef CRFP_ACT_BF16
                rc = round_bf16_copy(w, pk + it.off_w, (int)it.n_w, s);
#else
                if (hipMemcpyAsync(pk + it.off_w, w, it.n_w * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) rc = 1;
#endif
                if (!rc && hipMemcpyAsync(pk + it.off_b, b, it.n_b * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) rc = 1;
        }
        if (rc) return rc;
    }
    return 0;
}
// who: the entry point's name in its error texts
static int check_packed_size(const char* who, size_t total_floats, size_t packed_bytes) {
    if (packed_bytes < total_floats * sizeof(float)) { set_error("%s: packed buffer too small", who); return CRFP_E_WORKSPACE; }
    return 0;
}

// ------------------------------------------------------------------ per-thread stream tables
// The event pool of a slot, and how a slot's events and streams are released.  How events are handed out is the slot type's own business.
struct EventPool {
    std::vector<hipEvent_t> ev;
    bool ok = true;
    hipEvent_t event(size_t i) {   // event i, created with every one before it on first use
        while (ev.size() <= i) {
            hipEvent_t e;
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { ok = false; return nullptr; }
            ev.push_back(e);
        }
        return ev[i];
    }
    void destroy(hipStream_t* streams, int n) {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        ev.clear();
        for (int i = 0; i < n; ++i) { if (streams[i]) (void)hipStreamDestroy(streams[i]); streams[i] = nullptr; }
        ok = true;
    }
};
constexpr int kMaxDevices = 64;
static bool side_stream_enabled() {
    static const bool on = !(getenv("CRFP_SIDE_STREAM") && atoi(getenv("CRFP_SIDE_STREAM")) == 0);   // read once
    return on;
}
// One table of Slot (one per device) per host thread, taken on first use from a process-wide registry: crfp_shutdown() walks ALL tables, so
// the streams and events of worker threads that have exited are released as well (a thread_local destructor would have to call into the HIP
// runtime while the process may already be tearing it down).  A thread that exits hands its table back to a free list -- its destructor
// makes NO HIP call, it only has the slots forget() what belonged to the thread -- and the next new thread reuses it with its streams and
// events, so a thread-per-request host does not grow the registry by one table per thread.  The registry itself is heap-allocated and never
// destroyed: worker threads may outlive the static destructors.  One registry per Slot type -- and, the template having internal linkage, per
// library that holds a copy of this code: two libraries loaded into one process share nothing.
// Slot: forget() (no HIP call) and destroy().
namespace {
template <class Slot>
struct StreamTables {
    struct Table { Slot dev[kMaxDevices]; };
    struct Registry { std::mutex mu; std::vector<Table*> all, idle; };
    static Registry& registry() { static Registry* r = new Registry(); return *r; }
    struct Lease {
        Table* t = nullptr;
        ~Lease() {
            if (!t) return;
            for (int d = 0; d < kMaxDevices; ++d) t->dev[d].forget();   // the next owner starts clean
            Registry& r = registry();
            std::lock_guard<std::mutex> lk(r.mu);
            r.idle.push_back(t);
        }
    };
    // streams and events belong to the device that was current when they were created; a device index outside the table gets no slot
    // (the caller then runs its single-stream schedule) instead of aliasing another device's.  Creates no stream or event.
    static Slot* current() {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return nullptr;
        static thread_local Lease mine;
        if (!mine.t) {
            Registry& r = registry();
            std::lock_guard<std::mutex> lk(r.mu);
            if (!r.idle.empty()) { mine.t = r.idle.back(); r.idle.pop_back(); }
            else { mine.t = new Table(); r.all.push_back(mine.t); }
        }
        return &mine.t->dev[dev];
    }
    static void destroy_all() {   // caller: no engine call in flight on any thread
        Registry& r = registry();
        std::lock_guard<std::mutex> lk(r.mu);
        for (Table* t : r.all)
            for (int d = 0; d < kMaxDevices; ++d) t->dev[d].destroy();
    }
    static int count() {
        Registry& r = registry();
        std::lock_guard<std::mutex> lk(r.mu);
        return (int)r.all.size();
    }
};
}  // namespace

// ------------------------------------------------------------------ binding a launch
struct SrcBind { const float* p; long long bs; int pad = 0; };
struct DstBind { float* p; long long bs; int q0, q1; int pad = 0; };

// The plan of a packed MFMA item with this launch's tensors, its packed weights and the status word.  Everything else -- dstH / dstW,
// resid / flow / s3 and their batch strides, dst_f32, src_bgroup, the status-word mapping, strict -- stays at the plan's zeros for the caller
// to set.
static ConvArgs bind_conv(const Item& it, const float* packed, int N, int H, int W, const std::vector<SrcBind>& srcs, const std::vector<DstBind>& dsts,
                          unsigned* ovf) {
    ConvArgs a = it.c;
    for (size_t i = 0; i < srcs.size(); ++i) { a.src[i].p = srcs[i].p; a.src[i].bstride = srcs[i].bs; a.src[i].pad = srcs[i].pad; }
    a.ndst = (int)dsts.size();
    for (size_t i = 0; i < dsts.size(); ++i) {
        a.dst[i].p = dsts[i].p; a.dst[i].bstride = dsts[i].bs; a.dst[i].q0 = dsts[i].q0; a.dst[i].q1 = dsts[i].q1;
        a.dst[i].pad = dsts[i].pad;
    }
    a.N = N; a.H = H; a.W = W;
    a.wpk = packed + it.off_w;
    a.bpk = packed + it.off_b;
    a.wsplit = packed + it.off_s;
    a.ovf = ovf;
    return a;
}

}  // namespace CRFP_NS
