// Per-operator C-ABI entry points (NCHW tensors as the reference's Python operators pass them).
#include "crfp_common.h"

#include <cmath>
#include <cstring>

using namespace crfp;

static size_t q4_bytes(int n, int c, int h, int w) { return align_up((size_t)n * ((c + 3) / 4) * h * w * 16, 256); }
static size_t p4_guard(int w) { return align_up((size_t)(w + 2) * 16, 256); }  // zeroed guard in front of plane 0
static size_t p4_bytes(int n, int c, int h, int w) {
    return p4_guard(w) + align_up((size_t)n * ((c + 3) / 4) * (h + 1) * (w + 1) * 16, 256);
}

// offset [n,2,h,w] + mask [n,1,h,w] -> the compact quad (dy, dx, mask, 0) dcn3_kernel reads
__global__ void offmask3_pack_kernel(const float* __restrict__ offset, const float* __restrict__ mask, float* __restrict__ out, long long hw, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long n = i / hw, p = i - n * hw;
    reinterpret_cast<float4*>(out)[i] = make_float4(offset[(2 * n) * hw + p], offset[(2 * n + 1) * hw + p], mask[n * hw + p], 0.0f);
}

extern "C" {

size_t crfp_flow_warp_workspace_bytes(int n, int c, int h, int w) { return 2 * q4_bytes(n, c, h, w); }

int crfp_flow_warp_f32(const float* x, const float* flow, float* out, int n, int c, int h, int w, int padding_mode,
                       void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !flow || !out || n < 1 || c < 1 || h < 1 || w < 1) { set_error("flow_warp: bad argument"); return CRFP_E_BADARG; }
    if (padding_mode != CRFP_PAD_ZEROS && padding_mode != CRFP_PAD_BORDER) { set_error("flow_warp: padding_mode %d unsupported", padding_mode); return CRFP_E_UNSUPPORTED; }
    if (!workspace || workspace_bytes < crfp_flow_warp_workspace_bytes(n, c, h, w)) { set_error("flow_warp: workspace too small"); return CRFP_E_WORKSPACE; }
    hipStream_t s = (hipStream_t)stream;
    float* xin = (float*)workspace;
    float* xo = (float*)((char*)workspace + q4_bytes(n, c, h, w));
    const int nq = (c + 3) / 4;
    const long long bs = (long long)nq * h * w * 4;
    int rc = launch_nchw_to_q4(x, xin, n, c, h, w, 0, s);
    if (!rc) rc = launch_flow_warp_q4(xin, bs, flow, (long long)h * w * 2, xo, bs, n, nq, h, w, padding_mode == CRFP_PAD_BORDER, 0, s);
    if (!rc) rc = launch_q4_to_nchw(xo, out, n, c, h, w, 0, s);
    return rc;
}

size_t crfp_dcnv2_workspace_bytes(int n, int cin, int cout, int h, int w, int k, int dg) {
    if (cin == 32 && cout == 32 && dg == 8 && k == 3)
        return p4_bytes(n, 32, h, w) + q4_bytes(n, 32, h, w) + q4_bytes(n, 216, h, w) + align_up(36 * 2 * 32 * 4 * sizeof(float), 256);
    return 256;
}

int crfp_dcnv2_forward_f32(const float* x, const float* offset, const float* mask, const float* weight,
                           const float* bias, float* out, int n, int cin, int cout, int h, int w, int k, int pad,
                           int dil, int dg, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !offset || !mask || !weight || !bias || !out || n < 1 || h < 1 || w < 1) { set_error("dcnv2: bad argument"); return CRFP_E_BADARG; }
    if (k != 3 || pad != 1 || dil != 1) { set_error("dcnv2: only kernel 3, padding 1, dilation 1 (got %d,%d,%d)", k, pad, dil); return CRFP_E_UNSUPPORTED; }
    if (dg < 1 || cin % dg != 0 || cout < 1) { set_error("dcnv2: cin %d not divisible by deformable_groups %d", cin, dg); return CRFP_E_BADARG; }
    hipStream_t s = (hipStream_t)stream;
    if (cin == 32 && cout == 32 && dg == 8) {
        if (!workspace || workspace_bytes < crfp_dcnv2_workspace_bytes(n, cin, cout, h, w, k, dg)) { set_error("dcnv2: workspace too small"); return CRFP_E_WORKSPACE; }
        char* p = (char*)workspace;
        float* xq = (float*)(p + p4_guard(w)); p += p4_bytes(n, 32, h, w);   // P4: padded planes, guard + pads zeroed below
        float* oq = (float*)p; p += q4_bytes(n, 32, h, w);
        float* om = (float*)p; p += q4_bytes(n, 216, h, w);
        float* wpk = (float*)p;
        if (hipMemsetAsync((char*)xq - p4_guard(w), 0, p4_bytes(n, 32, h, w), s) != hipSuccess) { set_error("dcnv2: memset failed"); return 1; }
        int rc = launch_nchw_to_q4(x, xq, n, 32, h, w, 1, s);
        if (!rc) rc = launch_offmask_nchw_to_q4(offset, mask, om, n, 144, 72, h, w, s);
        if (!rc) rc = launch_dcn_g8_pack(weight, wpk, s);
        if (!rc) rc = launch_dcn_g8(xq, 8LL * (h + 1) * (w + 1) * 4, om, 54LL * h * w * 4, wpk, bias, oq, 8LL * h * w * 4, n, h, w, s);
        if (!rc) rc = launch_q4_to_nchw(oq, out, n, 32, h, w, 0, s);
        return rc;
    }
    return launch_dcn_generic(x, offset, mask, weight, bias, out, n, cin, cout, h, w, dg, s);
}

// ---- DCNv2 backward (dcn_backward.hip): the forward's domain up to 64 channels, every argument error before any HIP call
static int dcnv2_backward_domain(int n, int cin, int cout, int h, int w, int k, int pad, int dil, int dg) {
    if (n < 1 || cin < 1 || cout < 1 || h < 1 || w < 1 || dg < 1) { set_error("dcnv2_backward: bad argument (need n, cin, cout, h, w, dg >= 1)"); return CRFP_E_BADARG; }
    if (k != 3 || pad != 1 || dil != 1) { set_error("dcnv2_backward: only kernel 3, padding 1, dilation 1 (got %d,%d,%d)", k, pad, dil); return CRFP_E_UNSUPPORTED; }
    if (cin % dg != 0) { set_error("dcnv2_backward: cin %d not divisible by deformable_groups %d", cin, dg); return CRFP_E_UNSUPPORTED; }
    if (!dcn_backward_shape_ok(n, cin, cout, h, w, dg)) {
        set_error("dcnv2_backward: up to 64 channels, 65535 images, 262140 rows and 2^58 tensor elements (got cin %d, cout %d, n %d, h %d, w %d)", cin, cout, n, h, w);
        return CRFP_E_UNSUPPORTED;
    }
    return 0;
}

size_t crfp_dcnv2_backward_workspace_bytes(int n, int cin, int cout, int h, int w, int k, int dg) {
    if (dcnv2_backward_domain(n, cin, cout, h, w, k, 1, 1, dg)) return 0;
    return dcn_backward_workspace_bytes(n, cin, cout, h, w, dg);
}

int crfp_dcnv2_backward_f32(const float* x, const float* offset, const float* mask, const float* weight, const float* grad_out,
                            float* grad_x, float* grad_offset, float* grad_mask, float* grad_weight, float* grad_bias,
                            int n, int cin, int cout, int h, int w, int k, int pad, int dil, int dg,
                            void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !offset || !mask || !weight || !grad_out) { set_error("dcnv2_backward: null pointer (x, offset, mask, weight and grad_out are required)"); return CRFP_E_BADARG; }
    if (!grad_x && !grad_offset && !grad_mask && !grad_weight && !grad_bias) { set_error("dcnv2_backward: all five outputs are null (nothing to do)"); return CRFP_E_BADARG; }
    if (const int rc = dcnv2_backward_domain(n, cin, cout, h, w, k, pad, dil, dg)) return rc;
    if (!workspace || workspace_bytes < dcn_backward_workspace_bytes(n, cin, cout, h, w, dg)) { set_error("dcnv2_backward: workspace too small"); return CRFP_E_WORKSPACE; }
    return launch_dcn_backward(x, offset, mask, weight, grad_out, grad_x, grad_offset, grad_mask, grad_weight, grad_bias, n, cin, cout, h, w, dg,
                               0, workspace, (hipStream_t)stream);
}

// ---- the backward of crfp_dcnv2_shared_f32 (dcn_backward.hip in its shared form): 4 -> 4 only, the compact offset / mask and their gradients
static int dcnv2_shared_backward_domain(int n, int cin, int cout, int h, int w) {
    if (n < 1 || cin < 1 || cout < 1 || h < 1 || w < 1) { set_error("dcnv2_shared_backward: bad argument (need n, cin, cout, h, w >= 1)"); return CRFP_E_BADARG; }
    if (cin != 4 || cout != 4) { set_error("dcnv2_shared_backward: the shared-offset form is built for 4 -> 4 channels (got %d -> %d)", cin, cout); return CRFP_E_UNSUPPORTED; }
    if (!dcn_backward_shape_ok(n, 4, 4, h, w, 1)) {
        set_error("dcnv2_shared_backward: up to 65535 images, 262140 rows and 2^58 tensor elements (got n %d, h %d, w %d)", n, h, w);
        return CRFP_E_UNSUPPORTED;
    }
    return 0;
}

size_t crfp_dcnv2_shared_backward_workspace_bytes(int n, int c, int h, int w) {
    if (dcnv2_shared_backward_domain(n, c, c, h, w)) return 0;
    return dcn_backward_workspace_bytes(n, 4, 4, h, w, 1);
}

int crfp_dcnv2_shared_backward_f32(const float* x, const float* offset, const float* mask, const float* weight, const float* grad_out,
                                   float* grad_x, float* grad_offset, float* grad_mask, float* grad_weight, float* grad_bias,
                                   int n, int cin, int cout, int h, int w, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !offset || !mask || !weight || !grad_out) { set_error("dcnv2_shared_backward: null pointer (x, offset, mask, weight and grad_out are required)"); return CRFP_E_BADARG; }
    if (!grad_x && !grad_offset && !grad_mask && !grad_weight && !grad_bias) { set_error("dcnv2_shared_backward: all five outputs are null (nothing to do)"); return CRFP_E_BADARG; }
    if (const int rc = dcnv2_shared_backward_domain(n, cin, cout, h, w)) return rc;
    if (!workspace || workspace_bytes < dcn_backward_workspace_bytes(n, 4, 4, h, w, 1)) { set_error("dcnv2_shared_backward: workspace too small"); return CRFP_E_WORKSPACE; }
    return launch_dcn_backward(x, offset, mask, weight, grad_out, grad_x, grad_offset, grad_mask, grad_weight, grad_bias, n, 4, 4, h, w, 1, 1,
                               workspace, (hipStream_t)stream);
}

// ---- flow_warp backward (warp_backward.hip): every argument error before any HIP call
static int flow_warp_backward_domain(int n, int c, int h, int w, int padding_mode) {
    if (n < 1 || c < 1 || h < 1 || w < 1) { set_error("flow_warp_backward: bad argument (need n, c, h, w >= 1)"); return CRFP_E_BADARG; }
    if (padding_mode != CRFP_PAD_ZEROS && padding_mode != CRFP_PAD_BORDER) { set_error("flow_warp_backward: padding_mode %d unsupported", padding_mode); return CRFP_E_UNSUPPORTED; }
    if (!flow_warp_backward_shape_ok(n, c, h, w)) {
        set_error("flow_warp_backward: up to 65535 images, 262140 rows, 2^30 columns and 2^58 tensor elements (got n %d, c %d, h %d, w %d)", n, c, h, w);
        return CRFP_E_UNSUPPORTED;
    }
    return 0;
}

// the kernel needs no scratch; one aligned unit is reserved so that the call has the shape of every other one (query, allocate, pass)
size_t crfp_flow_warp_backward_workspace_bytes(int n, int c, int h, int w) {
    if (flow_warp_backward_domain(n, c, h, w, CRFP_PAD_ZEROS)) return 0;
    return 256;
}

static int flow_warp_backward_call(const float* x, const float* flow, const float* grad_out, float* grad_x, float* grad_flow, int n, int c, int h,
                                   int w, int padding_mode, int displaced, void* workspace, size_t workspace_bytes, void* stream) {
    if (!flow || !grad_out) { set_error("flow_warp_backward: null pointer (flow and grad_out are required)"); return CRFP_E_BADARG; }
    if (!grad_x && !grad_flow) { set_error("flow_warp_backward: both outputs are null (nothing to do)"); return CRFP_E_BADARG; }
    if (grad_flow && !x) { set_error("flow_warp_backward: null pointer (x is required for grad_flow)"); return CRFP_E_BADARG; }
    if (const int rc = flow_warp_backward_domain(n, c, h, w, padding_mode)) return rc;
    if (!workspace || workspace_bytes < 256) { set_error("flow_warp_backward: workspace too small"); return CRFP_E_WORKSPACE; }
    return launch_flow_warp_backward(x, flow, grad_out, grad_x, grad_flow, n, c, h, w, padding_mode == CRFP_PAD_BORDER, displaced, (hipStream_t)stream);
}

int crfp_flow_warp_backward_f32(const float* x, const float* flow, const float* grad_out, float* grad_x, float* grad_flow,
                                int n, int c, int h, int w, int padding_mode, void* workspace, size_t workspace_bytes, void* stream) {
    return flow_warp_backward_call(x, flow, grad_out, grad_x, grad_flow, n, c, h, w, padding_mode, 1, workspace, workspace_bytes, stream);
}

// measurement hook (tools/warp_backward_time.py): the same call with the LDS window of grad_x on the undisplaced tile (window = 0)
int crfp_flow_warp_backward_window_f32(const float* x, const float* flow, const float* grad_out, float* grad_x, float* grad_flow,
                                       int n, int c, int h, int w, int padding_mode, int window, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    if (window != 0 && window != 1) { set_error("flow_warp_backward: window %d (0: on the tile, 1: displaced by the centre flow)", window); return CRFP_E_BADARG; }
    return flow_warp_backward_call(x, flow, grad_out, grad_x, grad_flow, n, c, h, w, padding_mode, window, workspace, workspace_bytes, stream);
}

// ---- DCNv2 4 -> 4, one deformable group, ONE (dy, dx) and ONE mask per pixel shared by the 9 taps (the
// `offset_mask_shared_across_taps` form).  The reference builds this by tiling the 2 + 1 channels 9x before the DCNv2 call
// (model/CRFP.py:341-347); here they stay compact: offset [n,2,h,w], mask [n,1,h,w].
size_t crfp_dcnv2_shared_workspace_bytes(int n, int c, int h, int w) {
    if (n < 1 || c != 4 || h < 1 || w < 1) return 0;
    return p4_bytes(n, 4, h, w) + 2 * q4_bytes(n, 4, h, w);
}

int crfp_dcnv2_shared_f32(const float* x, const float* offset, const float* mask, const float* weight, const float* bias, float* out,
                          int n, int cin, int cout, int h, int w, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !offset || !mask || !weight || !bias || !out || n < 1 || h < 1 || w < 1) { set_error("dcnv2_shared: bad argument"); return CRFP_E_BADARG; }
    if (cin != 4 || cout != 4) { set_error("dcnv2_shared: the shared-offset form is built for 4 -> 4 channels (got %d -> %d)", cin, cout); return CRFP_E_UNSUPPORTED; }
    if (!workspace || workspace_bytes < crfp_dcnv2_shared_workspace_bytes(n, 4, h, w)) { set_error("dcnv2_shared: workspace too small"); return CRFP_E_WORKSPACE; }
    hipStream_t s = (hipStream_t)stream;
    char* p = (char*)workspace;
    float* xq = (float*)(p + p4_guard(w)); p += p4_bytes(n, 4, h, w);   // P4: padded plane, guard + pads zero
    float* om = (float*)p; p += q4_bytes(n, 4, h, w);
    float* oq = (float*)p;
    if (hipMemsetAsync((char*)xq - p4_guard(w), 0, p4_bytes(n, 4, h, w), s) != hipSuccess) { set_error("dcnv2_shared: memset failed"); return 1; }
    int rc = launch_nchw_to_q4(x, xq, n, 4, h, w, 1, s);
    if (!rc) {   // quad = (dy, dx, mask, 0)
        const long long hw = (long long)h * w, total = hw * n;
        offmask3_pack_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(offset, mask, om, hw, total);
        if (hipGetLastError() != hipSuccess) { set_error("dcnv2_shared: pack launch failed"); rc = 1; }
    }
    if (!rc) rc = launch_dcn3(xq, (long long)(h + 1) * (w + 1) * 4, om, (long long)h * w * 4, weight, bias, oq, (long long)h * w * 4, n, h, w, s);
    if (!rc) rc = launch_q4_to_nchw(oq, out, n, 4, h, w, 0, s);
    return rc;
}

// (cin = cout = 32, dg = 8) with the weights packed once: crfp_dcnv2_g8_pack_f32 -> crfp_dcnv2_g8_packed_f32
size_t crfp_dcnv2_g8_packed_bytes(void) { return align_up(36 * 2 * 32 * 4 * sizeof(float), 256); }

int crfp_dcnv2_g8_pack_f32(const float* weight, void* packed, size_t packed_bytes, void* stream) {
    if (!weight || !packed) { set_error("dcnv2_g8_pack: bad argument"); return CRFP_E_BADARG; }
    if (packed_bytes < crfp_dcnv2_g8_packed_bytes()) { set_error("dcnv2_g8_pack: packed buffer too small"); return CRFP_E_WORKSPACE; }
    return launch_dcn_g8_pack(weight, (float*)packed, (hipStream_t)stream);
}

int crfp_dcnv2_g8_packed_f32(const float* x, const float* offset, const float* mask, const void* packed, const float* bias, float* out,
                             int n, int h, int w, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !offset || !mask || !packed || !bias || !out || n < 1 || h < 1 || w < 1) { set_error("dcnv2_g8_packed: bad argument"); return CRFP_E_BADARG; }
    if (!workspace || workspace_bytes < crfp_dcnv2_workspace_bytes(n, 32, 32, h, w, 3, 8)) { set_error("dcnv2_g8_packed: workspace too small"); return CRFP_E_WORKSPACE; }
    hipStream_t s = (hipStream_t)stream;
    char* p = (char*)workspace;
    float* xq = (float*)(p + p4_guard(w)); p += p4_bytes(n, 32, h, w);
    float* oq = (float*)p; p += q4_bytes(n, 32, h, w);
    float* om = (float*)p;
    if (hipMemsetAsync((char*)xq - p4_guard(w), 0, p4_bytes(n, 32, h, w), s) != hipSuccess) { set_error("dcnv2_g8_packed: memset failed"); return 1; }
    int rc = launch_nchw_to_q4(x, xq, n, 32, h, w, 1, s);
    if (!rc) rc = launch_offmask_nchw_to_q4(offset, mask, om, n, 144, 72, h, w, s);
    if (!rc) rc = launch_dcn_g8(xq, 8LL * (h + 1) * (w + 1) * 4, om, 54LL * h * w * 4, (const float*)packed, bias, oq, 8LL * h * w * 4, n, h, w, s);
    if (!rc) rc = launch_q4_to_nchw(oq, out, n, 32, h, w, 0, s);
    return rc;
}

static ConvArgs api_conv_plan(int cin, int cout, int act, float post_scale) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.nsrc = 1;
    a.src[0].kind = SRC_NCHW;
    a.src[0].nch = cin;
    a.src[0].nq = (cin + 3) / 4;
    a.kq = a.src[0].nq;
    if (a.kq & 1) {
        a.src[1].kind = SRC_ZERO;
        a.src[1].nch = 1;
        a.src[1].nq = 1;
        a.src[1].cbase = cin;
        a.nsrc = 2;
        a.kq += 1;
    }
    a.cin_total = cin;
    a.cout = cout;
    a.store = ST_NCHW;
    a.act = act;
    a.post_scale = post_scale;
    a.ctiles = (cout + 31) / 32;
    return a;
}

size_t crfp_conv3x3_workspace_bytes(int n, int cin, int cout, int h, int w) {
    (void)n; (void)h; (void)w;
    ConvArgs a = api_conv_plan(cin, cout, 0, 1.0f);
    return align_up(conv_packed_weight_floats(a) * sizeof(float), 256) + align_up((size_t)a.ctiles * 32 * sizeof(float), 256);
}

// Weights packed once (crfp_conv3x3_pack_f32), reused by every crfp_conv3x3_packed_f32 call: the operator without the per-call repack
size_t crfp_conv3x3_packed_bytes(int cin, int cout) { return crfp_conv3x3_workspace_bytes(1, cin, cout, 1, 1); }

int crfp_conv3x3_pack_f32(const float* weight, const float* bias, int cin, int cout, void* packed, size_t packed_bytes, void* stream) {
    if (!weight || !packed || cin < 1 || cout < 1) { set_error("conv3x3_pack: bad argument"); return CRFP_E_BADARG; }
    if (packed_bytes < crfp_conv3x3_packed_bytes(cin, cout)) { set_error("conv3x3_pack: packed buffer too small"); return CRFP_E_WORKSPACE; }
    ConvArgs a = api_conv_plan(cin, cout, 0, 1.0f);
    float* wpk = (float*)packed;
    float* bpk = (float*)((char*)packed + align_up(conv_packed_weight_floats(a) * sizeof(float), 256));
    return launch_conv_pack(a, weight, bias, nullptr, nullptr, cout, wpk, bpk, (hipStream_t)stream);
}

int crfp_conv3x3_packed_f32(const float* x, const void* packed, float* out, int n, int cin, int cout, int h, int w, int act,
                            float post_scale, void* stream) {
    if (!x || !packed || !out || n < 1 || cin < 1 || cout < 1 || h < 1 || w < 1) { set_error("conv3x3_packed: bad argument"); return CRFP_E_BADARG; }
    if (act < CRFP_ACT_NONE || act > CRFP_ACT_SIGMOID) { set_error("conv3x3_packed: unknown activation %d", act); return CRFP_E_BADARG; }
    ConvArgs a = api_conv_plan(cin, cout, act, post_scale);
    a.src[0].p = x;
    a.src[0].bstride = (long long)cin * h * w;
    a.ndst = 1;
    a.dst[0].p = out;
    a.dst[0].bstride = (long long)cout * h * w;
    a.dst[0].q0 = 0;
    a.dst[0].q1 = (cout + 3) / 4;
    a.N = n; a.H = h; a.W = w;
    a.wpk = (const float*)packed;
    a.bpk = (const float*)((const char*)packed + align_up(conv_packed_weight_floats(a) * sizeof(float), 256));
    return launch_conv_mfma(a, "conv_mfma:api_nchw", (hipStream_t)stream);
}

int crfp_conv3x3_f32(const float* x, const float* weight, const float* bias, float* out, int n, int cin, int cout, int h,
                     int w, int act, float post_scale, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !weight || !out || n < 1 || cin < 1 || cout < 1 || h < 1 || w < 1) { set_error("conv3x3: bad argument"); return CRFP_E_BADARG; }
    if (act < CRFP_ACT_NONE || act > CRFP_ACT_SIGMOID) { set_error("conv3x3: unknown activation %d", act); return CRFP_E_BADARG; }
    if (!workspace || workspace_bytes < crfp_conv3x3_workspace_bytes(n, cin, cout, h, w)) { set_error("conv3x3: workspace too small"); return CRFP_E_WORKSPACE; }
    hipStream_t s = (hipStream_t)stream;
    ConvArgs a = api_conv_plan(cin, cout, act, post_scale);
    float* wpk = (float*)workspace;
    float* bpk = (float*)((char*)workspace + align_up(conv_packed_weight_floats(a) * sizeof(float), 256));
    int rc = launch_conv_pack(a, weight, bias, nullptr, nullptr, cout, wpk, bpk, s);
    if (rc) return rc;
    a.src[0].p = x;
    a.src[0].bstride = (long long)cin * h * w;
    a.ndst = 1;
    a.dst[0].p = out;
    a.dst[0].bstride = (long long)cout * h * w;
    a.dst[0].q0 = 0;
    a.dst[0].q1 = (cout + 3) / 4;
    a.N = n; a.H = h; a.W = w;
    a.wpk = wpk;
    a.bpk = bpk;
    return launch_conv_mfma(a, "conv_mfma:api_nchw", s);
}

// ---- the conv operator with everything SURVEY 8(b) lists for it: up to two inputs (a fused torch.cat), optional residual, activation,
// load through pixel_unshuffle(4), store plain into a channel slice of a wider tensor or through pixel_shuffle(r).
static ConvArgs api_conv_ex_plan(int cin, int cin2, int cout, int act, float post_scale, int unshuffle_r, int shuffle_r) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    int kq = 0;
    a.nsrc = 0;
    ConvSrc& s0 = a.src[a.nsrc++];
    s0.kind = unshuffle_r == 4 ? SRC_UNSHUF4 : SRC_NCHW;
    s0.nch = cin;
    s0.nq = unshuffle_r == 4 ? 16 * ((cin / 16 + 3) / 4) : (cin + 3) / 4;   // SRC_UNSHUF4: 16 sub-positions per hi-res quad
    s0.cbase = 0;
    kq += s0.nq;
    if (cin2 > 0) {
        ConvSrc& s1 = a.src[a.nsrc++];
        s1.kind = SRC_NCHW; s1.nch = cin2; s1.nq = (cin2 + 3) / 4; s1.cbase = cin;
        kq += s1.nq;
    }
    if (kq & 1) {
        ConvSrc& z = a.src[a.nsrc++];
        z.kind = SRC_ZERO; z.nch = 1; z.nq = 1; z.cbase = cin + cin2;
        kq += 1;
    }
    a.kq = kq;
    a.cin_total = cin + cin2;
    a.cout = cout;
    a.store = shuffle_r > 1 ? ST_PS : ST_NCHW;
    a.ps_r = shuffle_r > 1 ? shuffle_r : 0;
    a.act = act;
    a.post_scale = post_scale;
    a.ctiles = (conv_packed_rows(cout, a.store, a.ps_r) + 31) / 32;
    return a;
}

static bool conv_ex_args_ok(int cin, int cin2, int cout, int act, int unshuffle_r, int shuffle_r, bool has_resid) {
    if (cin < 1 || cin2 < 0 || cout < 1) { set_error("conv3x3_ex: bad channel counts (%d, %d -> %d)", cin, cin2, cout); return false; }
    if (act < CRFP_ACT_NONE || act > CRFP_ACT_SIGMOID) { set_error("conv3x3_ex: unknown activation %d", act); return false; }
    if (unshuffle_r != 0 && unshuffle_r != 1 && unshuffle_r != 4) { set_error("conv3x3_ex: pixel_unshuffle load supports r = 4 (got %d)", unshuffle_r); return false; }
    if (unshuffle_r == 4 && (cin2 > 0 || cin % 16)) { set_error("conv3x3_ex: pixel_unshuffle(4) load takes one input with cin %% 16 == 0"); return false; }
    if (shuffle_r != 0 && shuffle_r != 1 && shuffle_r != 2 && shuffle_r != 4) { set_error("conv3x3_ex: pixel_shuffle store supports r in {2, 4} (got %d)", shuffle_r); return false; }
    if (shuffle_r > 1 && (cout % (shuffle_r * shuffle_r) || has_resid || act == CRFP_ACT_TANH || act == CRFP_ACT_SIGMOID)) {
        set_error("conv3x3_ex: pixel_shuffle store needs cout %% r^2 == 0, no residual, activation none / relu / lrelu");
        return false;
    }
    return true;
}

size_t crfp_conv3x3_ex_workspace_bytes(int n, int cin, int cin2, int cout, int h, int w, int unshuffle_r, int shuffle_r, int has_residual) {
    if (n < 1 || h < 1 || w < 1 || !conv_ex_args_ok(cin, cin2, cout, CRFP_ACT_NONE, unshuffle_r, shuffle_r, false)) return 0;
    const ConvArgs a = api_conv_ex_plan(cin, cin2, cout, 0, 1.0f, unshuffle_r, shuffle_r);
    size_t b = align_up(conv_packed_weight_floats(a) * sizeof(float), 256) + align_up((size_t)a.ctiles * 32 * sizeof(float), 256);
    if (unshuffle_r == 4) b += q4_bytes(n, cin / 16, 4 * h, 4 * w);
    if (has_residual) b += q4_bytes(n, cout, h, w);
    if (shuffle_r > 1) b += q4_bytes(n, cout / (shuffle_r * shuffle_r), h * shuffle_r, w * shuffle_r);
    return b;
}

/* x: [n, cin, h, w]  (unshuffle_r = 4: [n, cin / 16, 4h, 4w], read as pixel_unshuffle(x, 4));  x2: optional [n, cin2, h, w];
 * weight [cout, cin + cin2, 3, 3];  residual: optional [n, cout, h, w], added after activation and post_scale;
 * out: [n, out_ctotal, h, w], channels [out_c0, out_c0 + cout) written (shuffle_r > 1: [n, cout / r^2, h r, w r], whole). */
int crfp_conv3x3_ex_f32(const float* x, int cin, const float* x2, int cin2, const float* weight, const float* bias, const float* residual,
                        float* out, int n, int cout, int h, int w, int act, float post_scale, int unshuffle_r, int shuffle_r,
                        int out_c0, int out_ctotal, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !weight || !out || n < 1 || h < 1 || w < 1 || (cin2 > 0 && !x2)) { set_error("conv3x3_ex: bad argument"); return CRFP_E_BADARG; }
    if (!conv_ex_args_ok(cin, cin2, cout, act, unshuffle_r, shuffle_r, residual != nullptr)) return CRFP_E_UNSUPPORTED;
    if (shuffle_r <= 1 && (out_c0 < 0 || out_ctotal < out_c0 + cout)) { set_error("conv3x3_ex: channel slice [%d, %d) outside %d channels", out_c0, out_c0 + cout, out_ctotal); return CRFP_E_BADARG; }
    if (!workspace || workspace_bytes < crfp_conv3x3_ex_workspace_bytes(n, cin, cin2, cout, h, w, unshuffle_r, shuffle_r, residual != nullptr)) {
        set_error("conv3x3_ex: workspace too small");
        return CRFP_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    ConvArgs a = api_conv_ex_plan(cin, cin2, cout, act, post_scale, unshuffle_r, shuffle_r);
    char* p = (char*)workspace;
    float* wpk = (float*)p; p += align_up(conv_packed_weight_floats(a) * sizeof(float), 256);
    float* bpk = (float*)p; p += align_up((size_t)a.ctiles * 32 * sizeof(float), 256);
    int rc = launch_conv_pack(a, weight, bias, nullptr, nullptr, cout, wpk, bpk, s);
    if (rc) return rc;
    if (unshuffle_r == 4) {   // the hi-res tensor as Q4, read through SRC_UNSHUF4
        float* xq = (float*)p; p += q4_bytes(n, cin / 16, 4 * h, 4 * w);
        rc = launch_nchw_to_q4(x, xq, n, cin / 16, 4 * h, 4 * w, 0, s);
        if (rc) return rc;
        a.src[0].p = xq;
        a.src[0].bstride = (long long)((cin / 16 + 3) / 4) * (4 * h) * (4 * w) * 4;
    } else {
        a.src[0].p = x;
        a.src[0].bstride = (long long)cin * h * w;
    }
    if (cin2 > 0) { a.src[1].p = x2; a.src[1].bstride = (long long)cin2 * h * w; }
    if (residual) {
        float* rq = (float*)p; p += q4_bytes(n, cout, h, w);
        rc = launch_nchw_to_q4(residual, rq, n, cout, h, w, 0, s);
        if (rc) return rc;
        a.resid = rq;
        a.resid_bstride = (long long)((cout + 3) / 4) * h * w * 4;
    }
    a.N = n; a.H = h; a.W = w;
    a.wpk = wpk; a.bpk = bpk;
    a.ndst = 1;
    if (shuffle_r > 1) {
        const int co = cout / (shuffle_r * shuffle_r), H2 = h * shuffle_r, W2 = w * shuffle_r;
        float* oq = (float*)p;
        a.dst[0].p = oq; a.dst[0].bstride = (long long)((co + 3) / 4) * H2 * W2 * 4; a.dst[0].q0 = 0; a.dst[0].q1 = (co + 3) / 4;
        a.dstH = H2; a.dstW = W2;
        rc = launch_conv_mfma(a, "conv_mfma:api_ex_ps", s);
        if (!rc) rc = launch_q4_to_nchw(oq, out, n, co, H2, W2, 0, s);
        return rc;
    }
    a.dst[0].p = out + (long long)out_c0 * h * w;
    a.dst[0].bstride = (long long)out_ctotal * h * w;
    a.dst[0].q0 = 0;
    a.dst[0].q1 = (cout + 3) / 4;
    return launch_conv_mfma(a, "conv_mfma:api_ex", s);
}

// ---- conv3x3_ex backward (conv_backward.hip): the forward's combination rules, every argument error before any HIP call
static int conv3x3_ex_backward_domain(int n, int cin, int cin2, int cout, int h, int w, int act, float post_scale, int unshuffle_r, int shuffle_r) {
    if (n < 1 || h < 1 || w < 1) { set_error("conv3x3_ex_backward: bad argument (need n, h, w >= 1)"); return CRFP_E_BADARG; }
    if (!conv_ex_args_ok(cin, cin2, cout, act, unshuffle_r, shuffle_r, false)) return CRFP_E_UNSUPPORTED;
    if ((act == CRFP_ACT_RELU || act == CRFP_ACT_LRELU01) && !(post_scale > 0.0f)) {
        set_error("conv3x3_ex_backward: relu / lrelu take their derivative from the sign of out and need post_scale > 0 (got %g)", (double)post_scale);
        return CRFP_E_UNSUPPORTED;
    }
    if ((act == CRFP_ACT_TANH || act == CRFP_ACT_SIGMOID) && !(post_scale < 0.0f || post_scale > 0.0f)) {   // also NaN
        set_error("conv3x3_ex_backward: tanh / sigmoid take their derivative from out / post_scale and need post_scale != 0 (got %g)", (double)post_scale);
        return CRFP_E_UNSUPPORTED;
    }
    if (cin > 1024 || cin2 > 1024 || !conv3x3_backward_shape_ok(n, cin + cin2, cout, h, w)) {
        set_error("conv3x3_ex_backward: up to 1024 input and 1024 output channels, 65535 images, 262140 rows, 2^30 columns and 2^58 tensor elements "
                  "(got cin %d + %d, cout %d, n %d, h %d, w %d)", cin, cin2, cout, n, h, w);
        return CRFP_E_UNSUPPORTED;
    }
    return 0;
}

size_t crfp_conv3x3_ex_backward_workspace_bytes(int n, int cin, int cin2, int cout, int h, int w, int unshuffle_r, int shuffle_r) {
    if (conv3x3_ex_backward_domain(n, cin, cin2, cout, h, w, CRFP_ACT_NONE, 1.0f, unshuffle_r, shuffle_r)) return 0;
    return conv3x3_backward_workspace_bytes(n, cin + cin2, cout, h, w);
}

int crfp_conv3x3_ex_backward_f32(const float* x, int cin, const float* x2, int cin2, const float* weight, const float* out,
                                 const float* grad_out, float* grad_x, float* grad_x2, float* grad_weight, float* grad_bias,
                                 int n, int cout, int h, int w, int act, float post_scale, int unshuffle_r, int shuffle_r,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    if (!grad_x && !grad_x2 && !grad_weight && !grad_bias) { set_error("conv3x3_ex_backward: all four outputs are null (nothing to do)"); return CRFP_E_BADARG; }
    if (!grad_out) { set_error("conv3x3_ex_backward: null pointer (grad_out is required)"); return CRFP_E_BADARG; }
    if (const int rc = conv3x3_ex_backward_domain(n, cin, cin2, cout, h, w, act, post_scale, unshuffle_r, shuffle_r)) return rc;
    if (act != CRFP_ACT_NONE && !out) { set_error("conv3x3_ex_backward: null pointer (out is required with an activation)"); return CRFP_E_BADARG; }
    if (grad_x2 && cin2 == 0) { set_error("conv3x3_ex_backward: grad_x2 without a second input (cin2 = 0)"); return CRFP_E_BADARG; }
    if (grad_weight && (!x || (cin2 > 0 && !x2))) { set_error("conv3x3_ex_backward: null pointer (x and x2 are required for grad_weight)"); return CRFP_E_BADARG; }
    if ((grad_x || grad_x2) && !weight) { set_error("conv3x3_ex_backward: null pointer (weight is required for grad_x / grad_x2)"); return CRFP_E_BADARG; }
    if (!workspace || workspace_bytes < conv3x3_backward_workspace_bytes(n, cin + cin2, cout, h, w)) { set_error("conv3x3_ex_backward: workspace too small"); return CRFP_E_WORKSPACE; }
    return launch_conv3x3_backward(x, cin, x2, cin2, weight, out, grad_out, grad_x, grad_x2, grad_weight, grad_bias, n, cout, h, w, act, post_scale,
                                   unshuffle_r, shuffle_r, workspace, (hipStream_t)stream);
}

int crfp_upsample_bilinear_f32(const float* x, float* out, int n, int c, int h, int w, int oh, int ow, float scale_h,
                               float scale_w, float mul, void* stream) {
    if (!x || !out || n < 1 || c < 1 || h < 1 || w < 1 || oh < 1 || ow < 1) { set_error("upsample: bad argument"); return CRFP_E_BADARG; }
    return launch_upsample_nchw(x, out, n, c, h, w, oh, ow, scale_h, scale_w, mul, (hipStream_t)stream);
}

int crfp_avgpool2_f32(const float* x, float* out, int n, int c, int h, int w, void* stream) {
    if (!x || !out || n < 1 || c < 1 || h < 2 || w < 2) { set_error("avgpool2: bad argument"); return CRFP_E_BADARG; }
    return launch_avgpool2_nchw(x, out, n, c, h, w, (hipStream_t)stream);
}

// ---- the backward passes of the resize and the pool, and the Charbonnier loss (train_backward.hip); every refusal before any HIP call
int crfp_upsample_bilinear_backward_f32(const float* grad_out, float* grad_x, int n, int c, int h, int w, int oh, int ow, float scale_h,
                                        float scale_w, float mul, void* stream) {
    if (!grad_out || !grad_x || n < 1 || c < 1 || h < 1 || w < 1 || oh < 1 || ow < 1) { set_error("upsample_backward: bad argument"); return CRFP_E_BADARG; }
    if (!(scale_h > 0.0f && scale_w > 0.0f && std::isfinite(scale_h) && std::isfinite(scale_w))) {
        set_error("upsample_backward: the source-index scales must be positive and finite");
        return CRFP_E_BADARG;
    }
    if (!train_backward_plane_shape_ok(n, c, h, w, oh, ow)) { set_error("upsample_backward: n * c > 65535, h > 262140 or more than 2^58 elements"); return CRFP_E_UNSUPPORTED; }
    return launch_upsample_bilinear_backward(grad_out, grad_x, n, c, h, w, oh, ow, scale_h, scale_w, mul, (hipStream_t)stream);
}

int crfp_avgpool2_backward_f32(const float* grad_out, float* grad_x, int n, int c, int h, int w, void* stream) {
    if (!grad_out || !grad_x || n < 1 || c < 1 || h < 2 || w < 2) { set_error("avgpool2_backward: bad argument"); return CRFP_E_BADARG; }
    if (!train_backward_plane_shape_ok(n, c, h, w, h / 2, w / 2)) { set_error("avgpool2_backward: n * c > 65535, h > 262140 or more than 2^58 elements"); return CRFP_E_UNSUPPORTED; }
    return launch_avgpool2_backward(grad_out, grad_x, n, c, h, w, (hipStream_t)stream);
}

static int charbonnier_domain(const char* who, int n, int c, int h, int w, const float* weight, int weight_c, float eps) {
    if (n < 1 || c < 1 || h < 1 || w < 1) { set_error("%s: bad argument (need n, c, h, w >= 1)", who); return CRFP_E_BADARG; }
    if (weight ? (weight_c != 1 && weight_c != c) : weight_c != 0) { set_error("%s: weight_c %d (0 with a null weight, else 1 or c = %d)", who, weight_c, c); return CRFP_E_BADARG; }
    if (!(eps >= 0.0f) || !std::isfinite(eps)) { set_error("%s: eps must be finite and >= 0", who); return CRFP_E_BADARG; }
    if (n > 65535 || (long long)h * w > (1LL << 58) / ((long long)n * c)) { set_error("%s: n > 65535 or more than 2^58 elements", who); return CRFP_E_UNSUPPORTED; }
    return 0;
}

size_t crfp_charbonnier_workspace_bytes(int n, int c, int h, int w) {
    if (n < 1 || c < 1 || h < 1 || w < 1 || n > 65535 || (long long)h * w > (1LL << 58) / ((long long)n * c)) return 0;
    return charbonnier_workspace_bytes(n, c, h, w);
}

int crfp_charbonnier_f32(const float* pred, const float* target, const float* weight, int weight_c, double* sums, int n, int c, int h, int w,
                         float eps, void* workspace, size_t workspace_bytes, void* stream) {
    if (!pred || !target || !sums) { set_error("charbonnier: null pointer"); return CRFP_E_BADARG; }
    if (const int rc = charbonnier_domain("charbonnier", n, c, h, w, weight, weight_c, eps)) return rc;
    if (!workspace || workspace_bytes < charbonnier_workspace_bytes(n, c, h, w)) { set_error("charbonnier: workspace too small"); return CRFP_E_WORKSPACE; }
    return launch_charbonnier(pred, target, weight, weight_c, sums, n, c, h, w, eps, workspace, (hipStream_t)stream);
}

int crfp_charbonnier_backward_f32(const float* pred, const float* target, const float* weight, int weight_c, const float* scale,
                                  float* grad_pred, int n, int c, int h, int w, float eps, void* stream) {
    if (!pred || !target || !scale || !grad_pred) { set_error("charbonnier_backward: null pointer"); return CRFP_E_BADARG; }
    if (const int rc = charbonnier_domain("charbonnier_backward", n, c, h, w, weight, weight_c, eps)) return rc;
    return launch_charbonnier_backward(pred, target, weight, weight_c, scale, grad_pred, n, c, h, w, eps, (hipStream_t)stream);
}

// fused a-15: conv_tttf on [state | x_hr], fovea blend, LeakyReLU -> new state; conv_last + bilinear x8 base -> frame
size_t crfp_fovea_head_workspace_bytes(int n, int h, int w) {
    const int H = 8 * h, W = 8 * w;
    return 4 * q4_bytes(n, 4, H, W) + align_up((size_t)n * 3 * H * W * sizeof(float), 256) + 2 * align_up((9 * 2 * 16 + 4) * sizeof(float), 256);
}

int crfp_fovea_head_f32(const float* state, const float* x_hr, const unsigned char* mask, const float* lr, const float* w_tttf,
                        const float* b_tttf, const float* w_last, const float* b_last, float* new_state, float* out, int n,
                        int h, int w, int y_only, void* workspace, size_t workspace_bytes, void* stream) {
    if (!state || !x_hr || !mask || !lr || !w_tttf || !b_tttf || !w_last || !b_last || !new_state || !out || n < 1 || h < 1 || w < 1) {
        set_error("fovea_head: bad argument");
        return CRFP_E_BADARG;
    }
    if (!workspace || workspace_bytes < crfp_fovea_head_workspace_bytes(n, h, w)) { set_error("fovea_head: workspace too small"); return CRFP_E_WORKSPACE; }
    hipStream_t s = (hipStream_t)stream;
    const int H = 8 * h, W = 8 * w;
    char* p = (char*)workspace;
    float* sq = (float*)p; p += q4_bytes(n, 4, H, W);
    float* xq = (float*)p; p += q4_bytes(n, 4, H, W);
    float* nq = (float*)p; p += q4_bytes(n, 4, H, W);
    float* bq = (float*)p; p += q4_bytes(n, 4, H, W);
    float* up = (float*)p; p += align_up((size_t)n * 3 * H * W * sizeof(float), 256);
    float* pk_t = (float*)p; p += align_up((9 * 2 * 16 + 4) * sizeof(float), 256);
    float* pk_l = (float*)p;
    const long long qs = (long long)H * W * 4;
    auto plan = [&](int nsrc, int cin, int cout, int epi) {
        NarrowArgs a;
        memset(&a, 0, sizeof(a));
        for (int i = 0; i < nsrc; ++i) { a.src[i].kind = SRC_Q4; a.src[i].nch = 4; a.src[i].nq = 1; a.src[i].cbase = 4 * i; a.src[i].bstride = qs; }
        a.nsrc = nsrc; a.kq = nsrc; a.cin_total = cin; a.cout = cout; a.act = CRFP_ACT_NONE; a.epi = epi; a.y_only = y_only;
        a.post_scale = 1.0f; a.N = n; a.H = H; a.W = W;
        return a;
    };
    NarrowArgs t = plan(2, 8, 4, NE_BLEND), l = plan(1, 4, y_only ? 1 : 3, NE_LAST);
    int rc = launch_nchw_to_q4(state, sq, n, 4, H, W, 0, s);
    if (!rc) rc = launch_nchw_to_q4(x_hr, xq, n, 4, H, W, 0, s);
    if (!rc) rc = launch_upsample_nchw(lr, up, n, 3, h, w, H, W, 0.125f, 0.125f, 1.0f, s);   // nn.Upsample(x8, bilinear, align_corners=False)
    if (!rc) rc = launch_nchw_to_q4(up, bq, n, 3, H, W, 0, s);
    if (!rc) rc = launch_narrow_pack(t, w_tttf, b_tttf, nullptr, nullptr, 0, pk_t, pk_t + 9 * 2 * 16, s);
    if (!rc) rc = launch_narrow_pack(l, w_last, b_last, nullptr, nullptr, 0, pk_l, pk_l + 9 * 1 * 16, s);
    if (rc) return rc;
    t.src[0].p = sq; t.src[1].p = xq; t.wpk = pk_t; t.bpk = pk_t + 9 * 2 * 16; t.dst = nq; t.dst_bstride = qs;
    t.mask = mask; t.mask_bstride = (long long)H * W;
    rc = launch_narrow(t, "conv_narrow:tttf_blend", s);
    l.src[0].p = nq; l.wpk = pk_l; l.bpk = pk_l + 9 * 1 * 16; l.dst = out; l.dst_bstride = (long long)(y_only ? 1 : 3) * H * W;
    l.base = bq; l.base_bstride = qs;
    if (!rc) rc = launch_narrow(l, "conv_narrow:last_plus_base", s);
    if (!rc) rc = launch_q4_to_nchw(nq, new_state, n, 4, H, W, 0, s);
    return rc;
}

int crfp_psnr_ssim_partial_f32(const float* a, const float* b, const unsigned char* mask, double* acc, int n, int c, int h, int w,
                               float mul, float add, void* stream) {
    if (!a || !b || !acc || n < 1 || c < 1 || h < 1 || w < 1) { set_error("psnr_ssim_partial: bad argument"); return CRFP_E_BADARG; }
    return launch_psnr_ssim_partial(a, b, mask, acc, n, c, h, w, mul, add, (hipStream_t)stream);
}

size_t crfp_window_scores_workspace_bytes(int n) { return window_scores_workspace_bytes(n); }

int crfp_window_scores_f32(const float* hr, const float* sr, float* psnr, float* ssim, int n, int c, int h, int w, int k, int stride,
                           void* workspace, size_t workspace_bytes, void* stream) {
    if (!hr || !sr || !psnr || !ssim) { set_error("window_scores: null pointer"); return CRFP_E_BADARG; }
    if (n < 1 || c < 1 || k < 1 || stride < 1 || k > h || k > w) { set_error("window_scores: bad argument (need n, c, k, stride >= 1 and k <= h, w)"); return CRFP_E_BADARG; }
    if (k > 16) { set_error("window_scores: kernel_size > 16 is not implemented"); return CRFP_E_UNSUPPORTED; }
    if (n > 65535) { set_error("window_scores: more than 65535 images per call"); return CRFP_E_UNSUPPORTED; }
    if (!workspace || workspace_bytes < crfp_window_scores_workspace_bytes(n)) { set_error("window_scores: workspace too small"); return CRFP_E_BADARG; }
    return launch_window_scores(hr, sr, psnr, ssim, n, c, h, w, k, stride, (float*)workspace, (hipStream_t)stream);
}

size_t crfp_frame_metrics_workspace_bytes(int n, int m, int h, int w) { return frame_metrics_workspace_bytes(n, m, h, w); }

int crfp_frame_metrics_f32(const float* sr, const float* hr, const uint8_t* masks, double* out, int n, int c, int m, int h, int w, int flags,
                           void* workspace, size_t workspace_bytes, void* stream) {
    if (!sr || !hr || !out) { set_error("frame_metrics: null pointer"); return CRFP_E_BADARG; }
    if (n < 1 || h < 1 || w < 1) { set_error("frame_metrics: bad argument (need n, h, w >= 1)"); return CRFP_E_BADARG; }
    if (c < 1 || c > 4) { set_error("frame_metrics: c must be 1..4, got %d", c); return CRFP_E_BADARG; }
    if (m < 0 || m > 7) { set_error("frame_metrics: m must be 0..7 masks, got %d", m); return CRFP_E_BADARG; }
    if (m > 0 && !masks) { set_error("frame_metrics: null masks with m = %d", m); return CRFP_E_BADARG; }
    if (flags & ~CRFP_METRICS_LUMA) { set_error("frame_metrics: unknown flags 0x%x", flags); return CRFP_E_BADARG; }
    if ((flags & CRFP_METRICS_LUMA) && c != 3) { set_error("frame_metrics: the LUMA flag needs c = 3, got %d", c); return CRFP_E_BADARG; }
    if (n > 65535 || h > 16 * 65535 || frame_metrics_tiles(h, w) > 0x7fffffffLL) {
        set_error("frame_metrics: more than 65535 frames per call or a frame beyond the launch grid"); return CRFP_E_UNSUPPORTED;
    }
    if (!workspace || workspace_bytes < crfp_frame_metrics_workspace_bytes(n, m, h, w)) { set_error("frame_metrics: workspace too small"); return CRFP_E_WORKSPACE; }
    return launch_frame_metrics(sr, hr, masks, out, n, c, m, h, w, flags & CRFP_METRICS_LUMA, workspace, (hipStream_t)stream);
}

int crfp_gaze_prep_f32(const float* gt, const int32_t* rows, float* fv, uint8_t* mk, uint8_t* regions, uint8_t* fg, int n, int c, int h, int w,
                       int dilate, void* stream) {
    if (!rows || !mk || !regions || !fg) { set_error("gaze_prep: null pointer (rows, mk, regions and fg are required)"); return CRFP_E_BADARG; }
    if ((gt == nullptr) != (fv == nullptr)) { set_error("gaze_prep: gt and fv go together (both given, or both null for the masks alone)"); return CRFP_E_BADARG; }
    if (n < 1 || c < 1 || h < 1 || w < 1) { set_error("gaze_prep: bad argument (need n, c, h, w >= 1)"); return CRFP_E_BADARG; }
    if (dilate < 0) { set_error("gaze_prep: dilate must be >= 0, got %d", dilate); return CRFP_E_BADARG; }
    return launch_gaze_prep(gt, rows, fv, mk, regions, fg, n, c, h, w, dilate, (hipStream_t)stream);
}

int crfp_frame_ingest_u8(const uint8_t* lr_u8, const uint8_t* crop_u8, const int32_t* rects, float* lr, float* fv, uint8_t* mk, int n, int h, int w,
                         int fh, int fw, int H, int W, int flags, void* stream) {
    if ((lr_u8 == nullptr) != (lr == nullptr)) { set_error("frame_ingest: lr_u8 and lr go together (both given, or both null for the fovea alone)"); return CRFP_E_BADARG; }
    const int fovea = (crop_u8 != nullptr) + (rects != nullptr) + (fv != nullptr) + (mk != nullptr);
    if (fovea != 0 && fovea != 4) { set_error("frame_ingest: crop_u8, rects, fv and mk go together (all given, or all null for the LR frame alone)"); return CRFP_E_BADARG; }
    if (!lr && !fovea) { set_error("frame_ingest: null pointer (nothing to do)"); return CRFP_E_BADARG; }
    if (n < 1 || h < 1 || w < 1 || fh < 1 || fw < 1 || H < 1 || W < 1) { set_error("frame_ingest: bad argument (need n, h, w, fh, fw, H, W >= 1)"); return CRFP_E_BADARG; }
    if (flags & ~CRFP_IO_BGR) { set_error("frame_ingest: unknown flags 0x%x (the BGR flag is the only one)", flags); return CRFP_E_BADARG; }
    return launch_frame_ingest(lr_u8, crop_u8, rects, lr, fv, mk, n, h, w, fh, fw, H, W, flags & CRFP_IO_BGR, (hipStream_t)stream);
}

int crfp_frame_export_u8(const float* sr, const float* chroma, uint8_t* out_u8, int n, int c, int H, int W, int flags, void* stream) {
    if (!sr || !out_u8) { set_error("frame_export: null pointer (sr and out_u8 are required)"); return CRFP_E_BADARG; }
    if (n < 1 || H < 1 || W < 1) { set_error("frame_export: bad argument (need n, H, W >= 1)"); return CRFP_E_BADARG; }
    if (c != 1 && c != 3) { set_error("frame_export: c must be 1 or 3, got %d", c); return CRFP_E_BADARG; }
    if (c == 3 && chroma) { set_error("frame_export: chroma goes with c = 1 (a luma frame); c = 3 takes none"); return CRFP_E_BADARG; }
    if (c == 1 && !chroma) { set_error("frame_export: c = 1 needs the chroma frame"); return CRFP_E_BADARG; }
    if (flags & ~CRFP_IO_BGR) { set_error("frame_export: unknown flags 0x%x (the BGR flag is the only one)", flags); return CRFP_E_BADARG; }
    return launch_frame_export(sr, chroma, out_u8, n, c, H, W, flags & CRFP_IO_BGR, (hipStream_t)stream);
}

int crfp_bicubic_taps(int in_size, int out_size, int32_t* bounds, int32_t* taps, int taps_capacity) {
    if (!bounds || !taps) { set_error("bicubic_taps: null pointer"); return CRFP_E_BADARG; }
    if (in_size < 1 || out_size < 1) { set_error("bicubic_taps: bad argument (need in_size, out_size >= 1)"); return CRFP_E_BADARG; }
    const long long ksize = bicubic_ksize(in_size, out_size);
    if (ksize * out_size > 0x7fffffffLL) { set_error("bicubic_taps: a table of %lld x %d taps does not fit an int", ksize, out_size); return CRFP_E_UNSUPPORTED; }
    if (taps_capacity < ksize * out_size) { set_error("bicubic_taps: taps holds %d ints, %lld x %d are needed", taps_capacity, ksize, out_size); return CRFP_E_WORKSPACE; }
    bicubic_taps_host(in_size, out_size, (int)ksize, bounds, taps);
    return (int)ksize;
}

size_t crfp_resize_bicubic_workspace_bytes(int n, int h, int w, int H, int W) { return bicubic_workspace_bytes(n, h, w, H, W); }

// the checks the two bicubic entry points share, after their pointers and flags
static int bicubic_check(const char* what, int n, int h, int w, int H, int W, const void* workspace, size_t workspace_bytes) {
    if (n < 1 || h < 1 || w < 1 || H < 1 || W < 1) { set_error("%s: bad argument (need n, h, w, H, W >= 1)", what); return CRFP_E_BADARG; }
    const size_t need = bicubic_workspace_bytes(n, h, w, H, W);
    if (!need) {
        set_error("%s: more than 65535 frames per call, tap tables beyond an int or a frame beyond the launch grid", what);
        return CRFP_E_UNSUPPORTED;
    }
    if (!workspace || workspace_bytes < need) { set_error("%s: workspace too small (%zu bytes, %zu are needed)", what, workspace ? workspace_bytes : (size_t)0, need); return CRFP_E_WORKSPACE; }
    if ((uintptr_t)workspace % 16) { set_error("%s: the workspace must be 16-byte aligned", what); return CRFP_E_BADARG; }
    return 0;
}

int crfp_resize_bicubic_u8(const uint8_t* src, void* dst, int n, int h, int w, int H, int W, int flags, void* workspace, size_t workspace_bytes,
                           void* stream) {
    if (!src || !dst) { set_error("resize_bicubic: null pointer (src and dst are required)"); return CRFP_E_BADARG; }
    if (flags & ~(CRFP_IO_BGR | CRFP_IO_OUT_F32 | CRFP_IO_TWO_PASS)) { set_error("resize_bicubic: unknown flags 0x%x", flags); return CRFP_E_BADARG; }
    if (const int rc = bicubic_check("resize_bicubic", n, h, w, H, W, workspace, workspace_bytes)) return rc;
    return launch_bicubic(src, dst, nullptr, n, h, w, H, W, flags & CRFP_IO_OUT_F32 ? BC_EPI_F32 : BC_EPI_U8, flags & CRFP_IO_BGR,
                          flags & CRFP_IO_TWO_PASS, workspace, (hipStream_t)stream);
}

int crfp_frame_export_y_bicubic_u8(const float* luma, const uint8_t* lr_u8, uint8_t* out_u8, int n, int h, int w, int H, int W, int flags,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    if (!luma || !lr_u8 || !out_u8) { set_error("frame_export_y_bicubic: null pointer (luma, lr_u8 and out_u8 are required)"); return CRFP_E_BADARG; }
    if (flags & ~CRFP_IO_BGR) { set_error("frame_export_y_bicubic: unknown flags 0x%x (the BGR flag is the only one)", flags); return CRFP_E_BADARG; }
    if (const int rc = bicubic_check("frame_export_y_bicubic", n, h, w, H, W, workspace, workspace_bytes)) return rc;
    return launch_bicubic(lr_u8, out_u8, luma, n, h, w, H, W, BC_EPI_MERGE, flags & CRFP_IO_BGR, 0, workspace, (hipStream_t)stream);
}

int crfp_psnr_partial_f32(const float* a, const float* b, double* acc, int n, int c, int h, int w, void* stream) {
    if (!a || !b || !acc || n < 1 || c < 1 || h < 1 || w < 1) { set_error("psnr_partial: bad argument"); return CRFP_E_BADARG; }
    return launch_psnr_partial(a, b, acc, n, c, h, w, (hipStream_t)stream);
}

}  // extern "C"
