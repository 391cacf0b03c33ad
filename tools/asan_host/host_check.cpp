// Host-logic check of the C-ABI under AddressSanitizer + UndefinedBehaviorSanitizer.
// Built by `make -C crfp_amd/csrc asan` from the library's sources compiled HOST-ONLY (hipcc --cuda-host-only -fsanitize=address,undefined):
// no device code, no GPU -- this runs in the CPU build container, never on the GPU box.  It drives what the library does on the host before
// any kernel is launched: workspace / packed-weight sizing (the Layout arenas of engine.hip / engine_rt.hip over many geometries and batch
// sizes), the parameter tables, and every argument-error path (tests/test_host_logic.py::test_argument_errors_do_not_touch_the_gpu,
// test_sizes_are_sane).  Exit code 0 = every expectation held and no sanitizer report was raised.
#include "../../include/crfp_hip.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <cstdint>
extern "C" long crfp_stub_launches(void);
extern "C" long crfp_stub_last_grid(int axis);   // the last launch's grid x / y / z (0 .. 2) and block x (3)

static int fails = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } \
    } while (0)

// `host_check precision`: the process runs with CRFP_PRECISION=f32 (the library reads the switch once per process, so it has to be there before the
// first call) and walks what the test hooks refuse under it: crfp_gather_probe has no dcn_g8 / dcn_fused launch to reach without the split-fp16 kernels
static int precision_refusals() {
    setenv("CRFP_PRECISION", "f32", 1);
    crfp_gather_args a;
    std::memset(&a, 0, sizeof(a));
    crfp_gather_report r;
    float* const p = reinterpret_cast<float*>(256);
    void* const wsp = reinterpret_cast<char*>(1ull << 40);
    a.x = a.x2 = a.aux = a.mask = a.flow = a.head_w = a.head_b = a.weight = a.bias = p;
    a.out = a.out2 = p;
    a.status = reinterpret_cast<unsigned*>(256);
    a.c = 32; a.n = 3; a.h = 9; a.w = 33;
    const long l0 = crfp_stub_launches();
    const struct { int mode; const char* text; } rows[] = {{CRFP_GPROBE_DCN_G8, "the engines' dcn_g8 runs on the split-fp16 image (no CRFP_PRECISION override)"},
                                                           {CRFP_GPROBE_DCN_FUSED, "the fused DCN launch needs the default conv / DCN kernels (no CRFP_PRECISION override)"}};
    for (const auto& row : rows) {
        a.mode = row.mode;
        EXPECT(crfp_gather_probe_workspace_bytes(&a) == 0 && std::strstr(crfp_last_error_string(), row.text) != nullptr);
        EXPECT(crfp_gather_probe_workspace_bytes_bf16(&a) == 0 && std::strstr(crfp_last_error_string(), row.text) != nullptr);
        EXPECT(crfp_gather_probe_plan(&a, &r) == CRFP_E_UNSUPPORTED && crfp_gather_probe_plan_bf16(&a, &r) == CRFP_E_UNSUPPORTED);
        EXPECT(crfp_gather_probe(&a, &r, wsp, 1 << 20, nullptr) == CRFP_E_UNSUPPORTED && crfp_gather_probe_bf16(&a, &r, wsp, 1 << 20, nullptr) == CRFP_E_UNSUPPORTED);
    }
    EXPECT(crfp_stub_launches() == l0);
    for (int mode : {CRFP_GPROBE_WARP, CRFP_GPROBE_WARP_DUAL, CRFP_GPROBE_DCN3, CRFP_GPROBE_DCN3_FUSED}) {   // the other modes do not depend on the switch
        a.mode = mode;
        const size_t bytes = crfp_gather_probe_workspace_bytes(&a), bytes16 = crfp_gather_probe_workspace_bytes_bf16(&a);
        EXPECT(bytes > 0 && bytes16 > 0 && crfp_gather_probe(&a, &r, wsp, bytes, nullptr) == 0 && crfp_gather_probe_bf16(&a, &r, wsp, bytes16, nullptr) == 0);
    }
    std::printf("host_check precision: %d failed expectations\n", fails);
    return fails ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "precision")) return precision_refusals();
    EXPECT(crfp_version() > 0);
    // ---- sizes (test_sizes_are_sane) over geometries incl. ragged and degenerate ones
    const size_t pw = crfp_dsv_packed_weight_bytes(0);
    EXPECT(pw > 9000000 && pw < 40000000);
    EXPECT(crfp_dsv_packed_weight_bytes(1) > 0 && crfp_dsv_packed_weight_bytes_bf16(0) > 0 && crfp_cra_packed_weight_bytes(0) > pw / 2);
    const size_t a = crfp_dsv_workspace_bytes(7, 180, 320), b = crfp_dsv_workspace_bytes(7, 270, 480);
    EXPECT(a > 1000000000ull && a < 4000000000ull && b > 2 * a && b < 5 * a / 2);
    EXPECT(crfp_dsv_workspace_bytes(0, 180, 320) == 0 && crfp_dsv_workspace_bytes(7, 4, 4) == 0);
    EXPECT(crfp_flow_warp_workspace_bytes(1, 32, 360, 640) == 2ull * 32 * 360 * 640 * 4);
    const int hs[] = {8, 9, 17, 20, 33, 64, 101, 180, 270}, ws[] = {8, 16, 26, 36, 47, 65, 130, 170, 320, 480};
    for (int h : hs)
        for (int w : ws)
            for (int t : {1, 2, 7, 33, 100}) {
                const size_t s1 = crfp_dsv_workspace_bytes(t, h, w), sb = crfp_dsv_workspace_bytes_bf16(t, h, w);
                EXPECT(s1 > 0 && sb > 0 && sb <= s1);
                EXPECT(crfp_dsv_status_offset(t, h, w) < s1 && crfp_dsv_status_offset_bf16(t, h, w) < sb);
                for (int n : {1, 2, 4, 65}) {
                    const size_t sn = crfp_dsv_batch_workspace_bytes(n, t, h, w);
                    EXPECT(sn >= s1 / 2 && crfp_dsv_batch_status_offset(n, t, h, w) + 4ull * n <= sn);
                    EXPECT(crfp_dsv_batch_workspace_bytes_bf16(n, t, h, w) > 0 && crfp_cra_batch_workspace_bytes(n, t, h, w) >= sn / 2);
                    EXPECT(crfp_cra_batch_status_offset(n, t, h, w) < crfp_cra_batch_workspace_bytes(n, t, h, w));
                    EXPECT(crfp_simple_batch_workspace_bytes(n, t, h, w) > sn && crfp_dense_batch_workspace_bytes_bf16(n, t, h, w) > 0);   // 8 feature quads per level instead of 6
                    EXPECT(crfp_simple_batch_status_offset(n, t, h, w) + 4ull * n <= crfp_simple_batch_workspace_bytes(n, t, h, w));
                }
            }
    EXPECT(crfp_dsv_batch_workspace_bytes(0, 7, 180, 320) == 0 && crfp_dsv_batch_workspace_bytes(-3, 7, 180, 320) == 0);
    EXPECT(crfp_conv3x3_workspace_bytes(1, 64, 32, 360, 640) > 0 && crfp_conv3x3_packed_bytes(64, 32) > 0 && crfp_dcnv2_g8_packed_bytes() > 0);
    EXPECT(crfp_conv3x3_ex_workspace_bytes(1, 32, 32, 32, 64, 64, 0, 2, 1) > 0);
    EXPECT(crfp_dcnv2_workspace_bytes(1, 32, 32, 360, 640, 3, 8) > 0 && crfp_dcnv2_shared_workspace_bytes(1, 4, 1440, 2560) > 0);
    EXPECT(crfp_spynet_workspace_bytes(1, 180, 320) > 0 && crfp_fovea_head_workspace_bytes(1, 1440, 2560) > 0);
    EXPECT(crfp_rt_packed_weight_bytes(0) > 0);
    EXPECT(crfp_rt_workspace_bytes(5, 135, 240, 96, 96, 720, 720) > 0);      // test_runtime.py's geometry
    EXPECT(crfp_rt_workspace_bytes(5, 135, 240, 2000, 96, 720, 720) == 0);   // fovea larger than the frame: bad geometry, reported
    EXPECT(crfp_rt_workspace_bytes(5, 135, 240, 96, 96, 724, 720) == 0);     // warp_size no multiple of 8
    // ---- the parameter tables
    int np = 0;
    while (crfp_dsv_param_name(np)) { EXPECT(crfp_dsv_param_numel(np, 0) > 0 && std::strlen(crfp_dsv_param_name(np)) > 3); ++np; }
    EXPECT(np == 118 && crfp_dsv_param_name(-1) == nullptr && crfp_dsv_param_numel(np, 0) <= 0);
    int nc = 0;
    while (crfp_cra_param_name(nc)) { EXPECT(crfp_cra_param_numel(nc, 0) > 0); ++nc; }
    EXPECT(nc > np);
    // CRFP_simple / CRFP: CRFP_DSV's names, four other shapes (upsample: 128 rows; upsample_post: 32 columns; dense: 96 / 12 columns in main.0)
    {
        int other_s = 0, other_d = 0;
        for (int i = 0; i < np; ++i) {
            EXPECT(crfp_simple_param_numel(i, 0) > 0 && crfp_dense_param_numel(i, 1) > 0);
            other_s += crfp_simple_param_numel(i, 0) != crfp_dsv_param_numel(i, 0);
            other_d += crfp_dense_param_numel(i, 0) != crfp_dsv_param_numel(i, 0);
        }
        EXPECT(other_s == 3 && other_d == 7 && crfp_simple_param_numel(np, 0) <= 0 && crfp_dense_param_numel(-1, 0) <= 0);
    }
    int nr = 0;
    while (crfp_rt_param_name(nr)) { EXPECT(crfp_rt_param_numel(nr, 0) > 0); ++nr; }
    EXPECT(nr > 0);
    // ---- argument errors: reported before anything touches the GPU (test_argument_errors_do_not_touch_the_gpu)
    float* const p16 = reinterpret_cast<float*>(16);   // a non-null, never dereferenced host-side pointer value
    EXPECT(crfp_dsv_forward_clip(nullptr, 0, nullptr, nullptr, nullptr, nullptr, 7, 180, 320, nullptr, 0, nullptr) == -1);
    EXPECT(std::strstr(crfp_last_error_string(), "null") != nullptr);
    EXPECT(crfp_flow_warp_f32(nullptr, nullptr, nullptr, 1, 4, 8, 8, 0, nullptr, 0, nullptr) == -1);
    EXPECT(crfp_dcnv2_forward_f32(p16, p16, p16, p16, p16, p16, 1, 32, 32, 8, 8, 5, 2, 1, 8, nullptr, 0, nullptr) == -3);
    EXPECT(std::strstr(crfp_last_error_string(), "kernel 3") != nullptr);
    EXPECT(crfp_dcnv2_forward_f32(p16, p16, p16, p16, p16, p16, 1, 30, 32, 8, 8, 3, 1, 1, 8, nullptr, 0, nullptr) == -1);
    EXPECT(crfp_conv3x3_f32(p16, p16, p16, p16, 1, 3, 8, 8, 8, 9, 1.0f, nullptr, 0, nullptr) == -1);
    // too small a workspace / bad dimensions on the engines: refused by the host-side checks
    const unsigned char* const m16 = reinterpret_cast<const unsigned char*>(16);
    EXPECT(crfp_dsv_forward_clip(p16, 0, p16, p16, m16, p16, 7, 180, 320, p16, 1024, nullptr) != 0);
    EXPECT(crfp_dsv_forward_clip(p16, 0, p16, p16, m16, p16, 0, 180, 320, p16, (size_t)1 << 40, nullptr) != 0);
    EXPECT(crfp_dsv_forward_batch(p16, 0, p16, p16, m16, p16, 0, 7, 180, 320, p16, (size_t)1 << 40, nullptr) != 0);
    EXPECT(crfp_dsv_forward_batch_bf16(p16, 0, p16, p16, m16, p16, 2, 7, 180, 320, p16, 64, nullptr) != 0);
    EXPECT(crfp_cra_forward_batch(p16, 0, p16, p16, m16, p16, 2, 7, 180, 320, p16, 64, nullptr) != 0);
    EXPECT(crfp_simple_forward_batch(p16, 0, p16, p16, m16, p16, 2, 7, 180, 320, p16, 64, nullptr) != 0);
    EXPECT(crfp_dense_forward_batch_bf16(p16, 0, p16, nullptr, m16, p16, 1, 7, 180, 320, p16, (size_t)1 << 40, nullptr) != 0);
    EXPECT(crfp_dsv_forward_clip_bf16(p16, CRFP_DSV_STRICT_F32, p16, p16, m16, p16, 7, 180, 320, p16, (size_t)1 << 40, nullptr) != 0);
    EXPECT(std::strlen(crfp_last_error_string()) > 0);
    // the window score maps: every refusal comes before the first launch
    {
        const size_t wsb = crfp_window_scores_workspace_bytes(2);
        const long l0 = crfp_stub_launches();
        EXPECT(wsb > 0 && crfp_window_scores_workspace_bytes(0) == 0 && crfp_window_scores_workspace_bytes(3) > wsb);
        EXPECT(crfp_window_scores_f32(nullptr, p16, p16, p16, 2, 3, 24, 31, 10, 5, p16, wsb, nullptr) == CRFP_E_BADARG);
        EXPECT(std::strstr(crfp_last_error_string(), "null") != nullptr);
        EXPECT(crfp_window_scores_f32(p16, nullptr, p16, p16, 2, 3, 24, 31, 10, 5, p16, wsb, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_window_scores_f32(p16, p16, nullptr, p16, 2, 3, 24, 31, 10, 5, p16, wsb, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_window_scores_f32(p16, p16, p16, nullptr, 2, 3, 24, 31, 10, 5, p16, wsb, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_window_scores_f32(p16, p16, p16, p16, 2, 3, 24, 31, 10, 5, nullptr, wsb, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_window_scores_f32(p16, p16, p16, p16, 2, 3, 24, 31, 10, 5, p16, wsb - 1, nullptr) == CRFP_E_BADARG);   // one byte short
        EXPECT(crfp_window_scores_f32(p16, p16, p16, p16, 0, 3, 24, 31, 10, 5, p16, wsb, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_window_scores_f32(p16, p16, p16, p16, 2, 0, 24, 31, 10, 5, p16, wsb, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_window_scores_f32(p16, p16, p16, p16, 2, 3, 24, 31, 0, 5, p16, wsb, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_window_scores_f32(p16, p16, p16, p16, 2, 3, 24, 31, 10, 0, p16, wsb, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_window_scores_f32(p16, p16, p16, p16, 2, 3, 9, 31, 10, 5, p16, wsb, nullptr) == CRFP_E_BADARG);        // k > h
        EXPECT(crfp_window_scores_f32(p16, p16, p16, p16, 2, 3, 24, 9, 10, 5, p16, wsb, nullptr) == CRFP_E_BADARG);        // k > w
        EXPECT(crfp_window_scores_f32(p16, p16, p16, p16, 2, 3, 24, 31, 17, 5, p16, wsb, nullptr) == CRFP_E_UNSUPPORTED);
        EXPECT(crfp_window_scores_f32(p16, p16, p16, p16, 2, 3, 8, 31, 17, 5, p16, wsb, nullptr) == CRFP_E_BADARG);        // k > h comes first
        EXPECT(crfp_stub_launches() == l0);
        // and accepted calls over the tile chooser's corners (stub runtime: nothing runs)
        for (int k : {1, 7, 10, 16})
            for (int st : {1, 5, 12, 1000})
                for (int c : {1, 3}) {
                    EXPECT(crfp_window_scores_f32(p16, p16, p16, p16, 2, c, 75, 130, k, st, p16, wsb, nullptr) == 0);
                    EXPECT(crfp_window_scores_f32(p16, p16, p16, p16, 1, c, 1072, 1920, k, st, p16, wsb, nullptr) == 0);
                    EXPECT(crfp_window_scores_f32(p16, p16, p16, p16, 1, c, k, k, k, st, p16, wsb, nullptr) == 0);
                }
        EXPECT(crfp_stub_launches() == l0 + 2 * 3 * 4 * 4 * 2);
    }
    // the frame metrics table: sizing, every refusal before the first launch, three launches per accepted call
    {
        const uint8_t* const k16 = reinterpret_cast<const uint8_t*>(16);
        double* const d16 = reinterpret_cast<double*>(16);
        const size_t probe = 256 * 4 * sizeof(float), cell = 5 * sizeof(double);
        EXPECT(crfp_frame_metrics_workspace_bytes(1, 0, 16, 64) == probe + cell);                  // exactly one tile
        EXPECT(crfp_frame_metrics_workspace_bytes(1, 0, 17, 65) == probe + 4 * cell);
        EXPECT(crfp_frame_metrics_workspace_bytes(5, 3, 70, 150) == 5 * (probe + 15 * 4 * cell));
        EXPECT(crfp_frame_metrics_workspace_bytes(1, 7, 1, 1) == probe + 8 * cell);
        EXPECT(crfp_frame_metrics_workspace_bytes(2, 3, 1440, 2560) == 2 * (probe + 3600 * 4 * cell));
        EXPECT(crfp_frame_metrics_workspace_bytes(0, 0, 8, 8) == 0 && crfp_frame_metrics_workspace_bytes(1, 8, 8, 8) == 0);
        EXPECT(crfp_frame_metrics_workspace_bytes(1, -1, 8, 8) == 0 && crfp_frame_metrics_workspace_bytes(1, 0, 0, 8) == 0);
        EXPECT(crfp_frame_metrics_workspace_bytes(1, 0, 8, -2) == 0);
        EXPECT(crfp_frame_metrics_workspace_bytes(1, 0, 2147483647, 2147483647) > 0);              // no overflow on the way to a size
        const size_t wsb = crfp_frame_metrics_workspace_bytes(2, 3, 24, 31);
        const long l0 = crfp_stub_launches();
        EXPECT(crfp_frame_metrics_f32(nullptr, p16, k16, d16, 2, 3, 3, 24, 31, 0, p16, wsb, nullptr) == CRFP_E_BADARG);
        EXPECT(std::strstr(crfp_last_error_string(), "null") != nullptr);
        EXPECT(crfp_frame_metrics_f32(p16, nullptr, k16, d16, 2, 3, 3, 24, 31, 0, p16, wsb, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_metrics_f32(p16, p16, k16, nullptr, 2, 3, 3, 24, 31, 0, p16, wsb, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_metrics_f32(p16, p16, nullptr, d16, 2, 3, 3, 24, 31, 0, p16, wsb, nullptr) == CRFP_E_BADARG);    // m > 0 without masks
        EXPECT(std::strstr(crfp_last_error_string(), "masks") != nullptr);
        EXPECT(crfp_frame_metrics_f32(p16, p16, k16, d16, 0, 3, 3, 24, 31, 0, p16, wsb, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_metrics_f32(p16, p16, k16, d16, 2, 0, 3, 24, 31, 0, p16, wsb, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_metrics_f32(p16, p16, k16, d16, 2, 5, 3, 24, 31, 0, p16, wsb, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_metrics_f32(p16, p16, k16, d16, 2, 3, -1, 24, 31, 0, p16, wsb, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_metrics_f32(p16, p16, k16, d16, 2, 3, 8, 24, 31, 0, p16, (size_t)1 << 30, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_metrics_f32(p16, p16, k16, d16, 2, 3, 3, 0, 31, 0, p16, wsb, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_metrics_f32(p16, p16, k16, d16, 2, 1, 3, 24, 31, CRFP_METRICS_LUMA, p16, wsb, nullptr) == CRFP_E_BADARG);
        EXPECT(std::strstr(crfp_last_error_string(), "LUMA") != nullptr);
        EXPECT(crfp_frame_metrics_f32(p16, p16, k16, d16, 2, 4, 3, 24, 31, CRFP_METRICS_LUMA, p16, wsb, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_metrics_f32(p16, p16, k16, d16, 2, 3, 3, 24, 31, 2, p16, wsb, nullptr) == CRFP_E_BADARG);        // unknown flag
        EXPECT(crfp_frame_metrics_f32(p16, p16, k16, d16, 2, 3, 3, 24, 31, 0, p16, wsb - 1, nullptr) == CRFP_E_WORKSPACE);  // one byte short
        EXPECT(crfp_frame_metrics_f32(p16, p16, k16, d16, 2, 3, 3, 24, 31, 0, nullptr, wsb, nullptr) == CRFP_E_WORKSPACE);
        EXPECT(crfp_frame_metrics_f32(p16, p16, k16, d16, 70000, 3, 0, 24, 31, 0, p16, (size_t)1 << 40, nullptr) == CRFP_E_UNSUPPORTED);
        EXPECT(crfp_stub_launches() == l0);
        int accepted = 0;
        for (int c : {1, 3, 4})
            for (int m : {0, 3, 7})
                for (const auto& g : {std::initializer_list<int>{1, 1}, {7, 9}, {16, 64}, {17, 65}, {1440, 2560}}) {
                    const int h = g.begin()[0], w = g.begin()[1];
                    const size_t need = crfp_frame_metrics_workspace_bytes(2, m, h, w);
                    EXPECT(crfp_frame_metrics_f32(p16, p16, m ? k16 : nullptr, d16, 2, c, m, h, w, c == 3 ? CRFP_METRICS_LUMA : 0, p16, need, nullptr) == 0);
                    ++accepted;
                }
        EXPECT(crfp_stub_launches() == l0 + 3 * accepted);
    }
    // the gaze rig's rectangle pass: every refusal before the first launch, one launch per accepted call, masks-only calls included
    {
        uint8_t* const k16 = reinterpret_cast<uint8_t*>(16);
        const int32_t* const r16 = reinterpret_cast<const int32_t*>(16);
        const long l0 = crfp_stub_launches();
        EXPECT(crfp_gaze_prep_f32(p16, nullptr, p16, k16, k16, k16, 2, 3, 24, 32, 10, nullptr) == CRFP_E_BADARG);
        EXPECT(std::strstr(crfp_last_error_string(), "null") != nullptr);
        EXPECT(crfp_gaze_prep_f32(p16, r16, p16, nullptr, k16, k16, 2, 3, 24, 32, 10, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_gaze_prep_f32(p16, r16, p16, k16, nullptr, k16, 2, 3, 24, 32, 10, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_gaze_prep_f32(p16, r16, p16, k16, k16, nullptr, 2, 3, 24, 32, 10, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_gaze_prep_f32(nullptr, r16, p16, k16, k16, k16, 2, 3, 24, 32, 10, nullptr) == CRFP_E_BADARG);   // fv without gt
        EXPECT(std::strstr(crfp_last_error_string(), "gt and fv") != nullptr);
        EXPECT(crfp_gaze_prep_f32(p16, r16, nullptr, k16, k16, k16, 2, 3, 24, 32, 10, nullptr) == CRFP_E_BADARG);   // gt without fv
        EXPECT(crfp_gaze_prep_f32(p16, r16, p16, k16, k16, k16, 0, 3, 24, 32, 10, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_gaze_prep_f32(p16, r16, p16, k16, k16, k16, 2, 0, 24, 32, 10, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_gaze_prep_f32(p16, r16, p16, k16, k16, k16, 2, 3, 0, 32, 10, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_gaze_prep_f32(p16, r16, p16, k16, k16, k16, 2, 3, 24, -1, 10, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_gaze_prep_f32(p16, r16, p16, k16, k16, k16, 2, 3, 24, 32, -1, nullptr) == CRFP_E_BADARG);
        EXPECT(std::strstr(crfp_last_error_string(), "dilate") != nullptr);
        EXPECT(crfp_gaze_prep_f32(p16, r16, p16, k16, k16, k16, 70000, 3, 24, 32, 10, nullptr) == CRFP_E_UNSUPPORTED);
        EXPECT(crfp_gaze_prep_f32(nullptr, r16, nullptr, k16, k16, k16, 1, 1, 2147483647, 2147483647, 10, nullptr) == CRFP_E_UNSUPPORTED);
        EXPECT(crfp_stub_launches() == l0);
        int accepted = 0;
        for (const auto& g : {std::initializer_list<int>{1, 1}, {23, 45}, {16, 64}, {1440, 2560}})
            for (int c : {1, 3})
                for (int masks_only : {0, 1})
                    for (uint8_t* m : {k16, reinterpret_cast<uint8_t*>(20)}) {   // 16-byte aligned and not: both kernel forms
                        EXPECT(crfp_gaze_prep_f32(masks_only ? nullptr : p16, r16, masks_only ? nullptr : p16, m, k16, k16, 2, c, g.begin()[0],
                                                  g.begin()[1], 10, nullptr) == 0);
                        ++accepted;
                    }
        EXPECT(crfp_stub_launches() == l0 + accepted);
    }
    // 8-bit frame I/O: every refusal before the first launch; an accepted ingest is one launch per half it was given, an export is one
    {
        uint8_t* const k16 = reinterpret_cast<uint8_t*>(16);
        const uint8_t* const c16 = reinterpret_cast<const uint8_t*>(16);
        const int32_t* const r16 = reinterpret_cast<const int32_t*>(16);
        const long l0 = crfp_stub_launches();
        EXPECT(crfp_frame_ingest_u8(nullptr, c16, r16, p16, p16, k16, 2, 24, 32, 8, 8, 192, 256, 0, nullptr) == CRFP_E_BADARG);   // lr without lr_u8
        EXPECT(std::strstr(crfp_last_error_string(), "lr_u8 and lr") != nullptr);
        EXPECT(crfp_frame_ingest_u8(c16, c16, r16, nullptr, p16, k16, 2, 24, 32, 8, 8, 192, 256, 0, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_ingest_u8(c16, nullptr, r16, p16, p16, k16, 2, 24, 32, 8, 8, 192, 256, 0, nullptr) == CRFP_E_BADARG);   // a part of the fovea group
        EXPECT(std::strstr(crfp_last_error_string(), "go together") != nullptr);
        EXPECT(crfp_frame_ingest_u8(c16, c16, nullptr, p16, p16, k16, 2, 24, 32, 8, 8, 192, 256, 0, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_ingest_u8(c16, c16, r16, p16, nullptr, k16, 2, 24, 32, 8, 8, 192, 256, 0, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_ingest_u8(c16, c16, r16, p16, p16, nullptr, 2, 24, 32, 8, 8, 192, 256, 0, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_ingest_u8(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 24, 32, 8, 8, 192, 256, 0, nullptr) == CRFP_E_BADARG);
        EXPECT(std::strstr(crfp_last_error_string(), "nothing to do") != nullptr);
        for (int pos = 0; pos < 7; ++pos) {
            int a[7] = {2, 24, 32, 8, 8, 192, 256};
            a[pos] = pos % 2 ? 0 : -1;
            EXPECT(crfp_frame_ingest_u8(c16, c16, r16, p16, p16, k16, a[0], a[1], a[2], a[3], a[4], a[5], a[6], 0, nullptr) == CRFP_E_BADARG);
            EXPECT(std::strstr(crfp_last_error_string(), "bad argument") != nullptr);
        }
        EXPECT(crfp_frame_ingest_u8(c16, c16, r16, p16, p16, k16, 2, 24, 32, 8, 8, 192, 256, 2, nullptr) == CRFP_E_BADARG);
        EXPECT(std::strstr(crfp_last_error_string(), "unknown flags") != nullptr);
        EXPECT(crfp_frame_ingest_u8(c16, c16, r16, p16, p16, k16, 70000, 24, 32, 8, 8, 192, 256, 0, nullptr) == CRFP_E_UNSUPPORTED);
        EXPECT(crfp_frame_ingest_u8(nullptr, c16, r16, nullptr, p16, k16, 1, 1, 1, 8, 8, 2147483647, 2147483647, 0, nullptr) == CRFP_E_UNSUPPORTED);
        EXPECT(crfp_frame_ingest_u8(c16, c16, r16, p16, p16, k16, 1, 2147483647, 2147483647, 8, 8, 192, 256, 0, nullptr) == CRFP_E_UNSUPPORTED);   // before its fovea half
        EXPECT(crfp_frame_export_u8(nullptr, nullptr, k16, 2, 3, 24, 32, 0, nullptr) == CRFP_E_BADARG);
        EXPECT(std::strstr(crfp_last_error_string(), "null") != nullptr);
        EXPECT(crfp_frame_export_u8(p16, nullptr, nullptr, 2, 3, 24, 32, 0, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_export_u8(p16, nullptr, k16, 0, 3, 24, 32, 0, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_export_u8(p16, nullptr, k16, 2, 3, -1, 32, 0, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_export_u8(p16, nullptr, k16, 2, 3, 24, 0, 0, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_export_u8(p16, nullptr, k16, 2, 2, 24, 32, 0, nullptr) == CRFP_E_BADARG);
        EXPECT(std::strstr(crfp_last_error_string(), "c must be 1 or 3") != nullptr);
        EXPECT(crfp_frame_export_u8(p16, p16, k16, 2, 3, 24, 32, 0, nullptr) == CRFP_E_BADARG);       // chroma with c = 3
        EXPECT(crfp_frame_export_u8(p16, nullptr, k16, 2, 1, 24, 32, 0, nullptr) == CRFP_E_BADARG);   // none with c = 1
        EXPECT(std::strstr(crfp_last_error_string(), "chroma") != nullptr);
        EXPECT(crfp_frame_export_u8(p16, nullptr, k16, 2, 3, 24, 32, 4, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_export_u8(p16, nullptr, k16, 70000, 3, 24, 32, 0, nullptr) == CRFP_E_UNSUPPORTED);
        EXPECT(crfp_frame_export_u8(p16, nullptr, k16, 1, 3, 2147483647, 2147483647, 0, nullptr) == CRFP_E_UNSUPPORTED);
        EXPECT(crfp_stub_launches() == l0);
        long launches = 0;
        for (const auto& g : {std::initializer_list<int>{1, 1}, {7, 9}, {16, 64}, {180, 320}})
            for (int flags : {0, CRFP_IO_BGR})
                for (uint8_t* m : {k16, reinterpret_cast<uint8_t*>(17)}) {   // aligned and not: both kernel forms
                    const int h = g.begin()[0], w = g.begin()[1];
                    EXPECT(crfp_frame_ingest_u8(c16, c16, r16, p16, p16, m, 2, h, w, 96, 96, 8 * h, 8 * w, flags, nullptr) == 0);
                    EXPECT(crfp_frame_ingest_u8(c16, nullptr, nullptr, p16, nullptr, nullptr, 2, h, w, 96, 96, 8 * h, 8 * w, flags, nullptr) == 0);
                    EXPECT(crfp_frame_ingest_u8(nullptr, c16, r16, nullptr, p16, m, 2, h, w, 96, 96, 8 * h, 8 * w, flags, nullptr) == 0);
                    EXPECT(crfp_frame_export_u8(p16, nullptr, m, 2, 3, 8 * h, 8 * w, flags, nullptr) == 0);
                    EXPECT(crfp_frame_export_u8(p16, p16, m, 2, 1, 8 * h, 8 * w, flags, nullptr) == 0);
                    launches += 2 + 1 + 1 + 1 + 1;
                }
        EXPECT(crfp_stub_launches() == l0 + launches);
    }
    // the bicubic resize: the host tap tables into exactly sized heap blocks (one int short is refused and nothing is written), sizing, every
    // refusal before the first launch; an accepted resize is the table kernel plus one fused launch or two passes, a merge table + fused
    {
        const int axes[][2] = {{1, 8}, {180, 1440}, {96, 12}};
        for (const auto& ax : axes) {
            const int in = ax[0], out = ax[1], ks = in > out ? 33 : 5;   // 96 -> 12: support 16
            int32_t* bounds = static_cast<int32_t*>(std::malloc(sizeof(int32_t) * 2 * out));
            int32_t* taps = static_cast<int32_t*>(std::malloc(sizeof(int32_t) * ks * out));
            int32_t* small = static_cast<int32_t*>(std::malloc(sizeof(int32_t) * (ks * out - 1)));
            EXPECT(crfp_bicubic_taps(in, out, bounds, small, ks * out - 1) == CRFP_E_WORKSPACE);   // a capacity one too small
            EXPECT(crfp_bicubic_taps(in, out, bounds, taps, ks * out) == ks);
            for (int xx = 0; xx < out; ++xx) {
                const int x0 = bounds[2 * xx], cnt = bounds[2 * xx + 1];
                long long sum = 0;
                for (int k = 0; k < ks; ++k) sum += taps[ks * xx + k];
                EXPECT(x0 >= 0 && cnt >= 1 && cnt <= ks && x0 + cnt <= in);
                EXPECT(sum > (1 << 22) - ks && sum < (1 << 22) + ks);       // normalised taps, each rounded once
                for (int k = cnt; k < ks; ++k) EXPECT(taps[ks * xx + k] == 0);
            }
            std::free(bounds); std::free(taps); std::free(small);
        }
        int32_t b2[2], k5[5];
        EXPECT(crfp_bicubic_taps(1, 1, nullptr, k5, 5) == CRFP_E_BADARG && crfp_bicubic_taps(1, 1, b2, nullptr, 5) == CRFP_E_BADARG);
        EXPECT(crfp_bicubic_taps(0, 1, b2, k5, 5) == CRFP_E_BADARG && crfp_bicubic_taps(1, -1, b2, k5, 5) == CRFP_E_BADARG);
        EXPECT(crfp_bicubic_taps(2147483647, 1, b2, k5, 5) == CRFP_E_UNSUPPORTED && crfp_bicubic_taps(2147483647, 2147483647, b2, k5, 5) == CRFP_E_UNSUPPORTED);
        EXPECT(crfp_bicubic_taps(1, 1, b2, k5, 5) == 5 && b2[0] == 0 && b2[1] == 1 && k5[0] == 1 << 22);
        uint8_t* const k16 = reinterpret_cast<uint8_t*>(16);
        const uint8_t* const c16 = reinterpret_cast<const uint8_t*>(16);
        const size_t need = crfp_resize_bicubic_workspace_bytes(2, 180, 320, 1440, 2560);
        EXPECT(need == 4ull * 7 * (1440 + 2560) + 2ull * 180 * 2560 * 3);
        EXPECT(crfp_resize_bicubic_workspace_bytes(0, 8, 8, 8, 8) == 0 && crfp_resize_bicubic_workspace_bytes(1, 8, 0, 8, 8) == 0);
        EXPECT(crfp_resize_bicubic_workspace_bytes(70000, 8, 8, 8, 8) == 0 && crfp_resize_bicubic_workspace_bytes(1, 2147483647, 8, 1, 8) == 0);
        EXPECT(crfp_resize_bicubic_workspace_bytes(1, 2147483647, 2147483647, 2147483647, 2147483647) == 0);
        const long l0 = crfp_stub_launches();
        EXPECT(crfp_resize_bicubic_u8(nullptr, k16, 2, 180, 320, 1440, 2560, 0, k16, need, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_resize_bicubic_u8(c16, nullptr, 2, 180, 320, 1440, 2560, 0, k16, need, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_resize_bicubic_u8(c16, k16, 2, 0, 320, 1440, 2560, 0, k16, need, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_resize_bicubic_u8(c16, k16, 2, 180, 320, 1440, 2560, 8, k16, need, nullptr) == CRFP_E_BADARG);
        EXPECT(std::strstr(crfp_last_error_string(), "unknown flags") != nullptr);
        EXPECT(crfp_resize_bicubic_u8(c16, k16, 2, 180, 320, 1440, 2560, 0, k16, need - 1, nullptr) == CRFP_E_WORKSPACE);
        EXPECT(crfp_resize_bicubic_u8(c16, k16, 2, 180, 320, 1440, 2560, 0, nullptr, need, nullptr) == CRFP_E_WORKSPACE);
        EXPECT(crfp_resize_bicubic_u8(c16, k16, 2, 180, 320, 1440, 2560, 0, reinterpret_cast<void*>(20), need, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_resize_bicubic_u8(c16, k16, 70000, 180, 320, 1440, 2560, 0, k16, (size_t)1 << 44, nullptr) == CRFP_E_UNSUPPORTED);
        EXPECT(crfp_frame_export_y_bicubic_u8(nullptr, c16, k16, 2, 180, 320, 1440, 2560, 0, k16, need, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_export_y_bicubic_u8(p16, nullptr, k16, 2, 180, 320, 1440, 2560, 0, k16, need, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_export_y_bicubic_u8(p16, c16, nullptr, 2, 180, 320, 1440, 2560, 0, k16, need, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_export_y_bicubic_u8(p16, c16, k16, 2, 180, 320, 1440, 2560, CRFP_IO_OUT_F32, k16, need, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_frame_export_y_bicubic_u8(p16, c16, k16, 2, 180, 320, 1440, 2560, 0, k16, need - 1, nullptr) == CRFP_E_WORKSPACE);
        EXPECT(crfp_frame_export_y_bicubic_u8(p16, c16, k16, 2, 180, 320, 179, 2560, 0, k16, (size_t)1 << 40, nullptr) == CRFP_E_UNSUPPORTED);   // shrinks along y
        EXPECT(std::strstr(crfp_last_error_string(), "fused path") != nullptr);
        EXPECT(crfp_stub_launches() == l0);
        long launches = 0;
        for (const auto& g : {std::initializer_list<int>{1, 1, 8, 8}, {17, 23, 136, 184}, {9, 11, 10, 13}, {64, 96, 8, 12}, {180, 320, 1440, 2560}})
            for (int flags : {0, CRFP_IO_BGR, CRFP_IO_OUT_F32, CRFP_IO_OUT_F32 | CRFP_IO_BGR | CRFP_IO_TWO_PASS})
                for (uint8_t* d : {k16, reinterpret_cast<uint8_t*>(17)}) {   // aligned and not: both kernel forms
                    const int h = g.begin()[0], w = g.begin()[1], H = g.begin()[2], W = g.begin()[3];
                    const size_t ws = crfp_resize_bicubic_workspace_bytes(2, h, w, H, W);
                    const bool fused = H >= h && W >= w;
                    EXPECT(ws > 0 && crfp_resize_bicubic_u8(c16, d, 2, h, w, H, W, flags, k16, ws, nullptr) == 0);
                    launches += fused && !(flags & CRFP_IO_TWO_PASS) ? 2 : 3;
                    if (fused && !(flags & ~CRFP_IO_BGR)) {
                        EXPECT(crfp_frame_export_y_bicubic_u8(p16, c16, d, 2, h, w, H, W, flags, k16, ws, nullptr) == 0);
                        launches += 2;
                    }
                }
        EXPECT(crfp_stub_launches() == l0 + launches);
    }
    // the conv3x3_ex backward: sizing, every refusal before the first launch, the launches each subset of wanted outputs takes
    {
        const size_t need = crfp_conv3x3_ex_backward_workspace_bytes(2, 5, 3, 7, 9, 11, 0, 0);
        EXPECT(need > 0 && crfp_conv3x3_ex_backward_workspace_bytes(1, 66, 0, 32, 360, 640, 0, 0) > 0);
        EXPECT(crfp_conv3x3_ex_backward_workspace_bytes(1, 4, 4, 4, 1440, 2560, 0, 0) > 0 && crfp_conv3x3_ex_backward_workspace_bytes(1, 128, 32, 288, 180, 320, 0, 0) > 0);
        EXPECT(crfp_conv3x3_ex_backward_workspace_bytes(1, 32, 0, 9, 5, 7, 4, 0) > 0 && crfp_conv3x3_ex_backward_workspace_bytes(1, 8, 0, 32, 5, 6, 0, 4) > 0);
        EXPECT(crfp_conv3x3_ex_backward_workspace_bytes(0, 5, 3, 7, 9, 11, 0, 0) == 0 && crfp_conv3x3_ex_backward_workspace_bytes(2, 0, 3, 7, 9, 11, 0, 0) == 0);
        EXPECT(crfp_conv3x3_ex_backward_workspace_bytes(2, 5, -1, 7, 9, 11, 0, 0) == 0 && crfp_conv3x3_ex_backward_workspace_bytes(2, 5, 3, 0, 9, 11, 0, 0) == 0);
        EXPECT(crfp_conv3x3_ex_backward_workspace_bytes(2, 5, 3, 7, 0, 11, 0, 0) == 0 && crfp_conv3x3_ex_backward_workspace_bytes(2, 5, 3, 7, 9, -4, 0, 0) == 0);
        EXPECT(crfp_conv3x3_ex_backward_workspace_bytes(2, 5, 3, 7, 9, 11, 2, 0) == 0 && crfp_conv3x3_ex_backward_workspace_bytes(2, 5, 3, 7, 9, 11, 0, 3) == 0);
        EXPECT(crfp_conv3x3_ex_backward_workspace_bytes(2, 24, 0, 7, 9, 11, 4, 0) == 0 && crfp_conv3x3_ex_backward_workspace_bytes(2, 16, 16, 7, 9, 11, 4, 0) == 0);
        EXPECT(crfp_conv3x3_ex_backward_workspace_bytes(2, 5, 3, 7, 9, 11, 0, 2) == 0);   // cout % 4
        EXPECT(crfp_conv3x3_ex_backward_workspace_bytes(2, 1000, 25, 7, 9, 11, 0, 0) == 0 && crfp_conv3x3_ex_backward_workspace_bytes(2, 5, 3, 1025, 9, 11, 0, 0) == 0);
        EXPECT(crfp_conv3x3_ex_backward_workspace_bytes(2, 2147483647, 2147483647, 7, 9, 11, 0, 0) == 0);
        EXPECT(crfp_conv3x3_ex_backward_workspace_bytes(70000, 5, 3, 7, 9, 11, 0, 0) == 0 && crfp_conv3x3_ex_backward_workspace_bytes(1, 5, 3, 7, 300000, 1, 0, 0) == 0);
        EXPECT(crfp_conv3x3_ex_backward_workspace_bytes(1, 5, 3, 7, 9, (1 << 30) + 1, 0, 0) == 0);
        EXPECT(crfp_conv3x3_ex_backward_workspace_bytes(65535, 1024, 0, 1024, 262140, 1 << 30, 0, 0) == 0);   // element counts beyond 64-bit indexing
        EXPECT(crfp_conv3x3_ex_backward_workspace_bytes(8, 64, 64, 64, 4320, 7680, 0, 0) > 0 && crfp_conv3x3_ex_backward_workspace_bytes(1, 1, 0, 1, 262140, 100000, 0, 0) > 0);
        const long l0 = crfp_stub_launches();
#define CVB(X, X2, W, OUT, GO, GX, GX2, GW, GB, N, CIN, CIN2, COUT, ACT, S, UR, SR, WS, WSB) \
    crfp_conv3x3_ex_backward_f32(X, CIN, X2, CIN2, W, OUT, GO, GX, GX2, GW, GB, N, COUT, 9, 11, ACT, S, UR, SR, WS, WSB, nullptr)
        EXPECT(CVB(p16, p16, p16, p16, p16, nullptr, nullptr, nullptr, nullptr, 2, 5, 3, 7, 2, 0.5f, 0, 0, p16, need) == CRFP_E_BADARG);
        EXPECT(std::strstr(crfp_last_error_string(), "nothing to do") != nullptr);
        EXPECT(CVB(p16, p16, p16, p16, nullptr, p16, p16, p16, p16, 2, 5, 3, 7, 2, 0.5f, 0, 0, p16, need) == CRFP_E_BADARG);
        EXPECT(std::strstr(crfp_last_error_string(), "null") != nullptr);
        EXPECT(CVB(p16, p16, p16, nullptr, p16, p16, p16, p16, p16, 2, 5, 3, 7, 2, 0.5f, 0, 0, p16, need) == CRFP_E_BADARG);     // out with an activation
        EXPECT(CVB(nullptr, p16, p16, p16, p16, p16, p16, p16, p16, 2, 5, 3, 7, 2, 0.5f, 0, 0, p16, need) == CRFP_E_BADARG);     // x for grad_weight
        EXPECT(CVB(p16, nullptr, p16, p16, p16, p16, p16, p16, p16, 2, 5, 3, 7, 2, 0.5f, 0, 0, p16, need) == CRFP_E_BADARG);     // x2 for grad_weight
        EXPECT(CVB(p16, p16, nullptr, p16, p16, p16, p16, p16, p16, 2, 5, 3, 7, 2, 0.5f, 0, 0, p16, need) == CRFP_E_BADARG);     // weight for grad_x
        EXPECT(CVB(p16, nullptr, p16, p16, p16, p16, p16, p16, p16, 2, 8, 0, 7, 2, 0.5f, 0, 0, p16, need) == CRFP_E_BADARG);     // grad_x2 without x2
        EXPECT(CVB(p16, p16, p16, p16, p16, p16, p16, p16, p16, 0, 5, 3, 7, 2, 0.5f, 0, 0, p16, need) == CRFP_E_BADARG);
        EXPECT(CVB(p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 0, 3, 7, 2, 0.5f, 0, 0, p16, need) == CRFP_E_UNSUPPORTED);    // the forward's rules
        EXPECT(CVB(p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 5, 3, 7, 5, 0.5f, 0, 0, p16, need) == CRFP_E_UNSUPPORTED);
        EXPECT(std::strstr(crfp_last_error_string(), "activation") != nullptr);
        EXPECT(CVB(p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 5, 3, 7, 2, 0.5f, 2, 0, p16, need) == CRFP_E_UNSUPPORTED);
        EXPECT(CVB(p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 5, 3, 8, 3, 0.5f, 0, 2, p16, need) == CRFP_E_UNSUPPORTED);    // tanh with a shuffle store
        EXPECT(CVB(p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 5, 3, 7, 1, 0.0f, 0, 0, p16, need) == CRFP_E_UNSUPPORTED);
        EXPECT(std::strstr(crfp_last_error_string(), "post_scale > 0") != nullptr);
        EXPECT(CVB(p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 5, 3, 7, 2, -1.0f, 0, 0, p16, need) == CRFP_E_UNSUPPORTED);
        EXPECT(CVB(p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 5, 3, 7, 3, 0.0f, 0, 0, p16, need) == CRFP_E_UNSUPPORTED);
        EXPECT(std::strstr(crfp_last_error_string(), "post_scale != 0") != nullptr);
        EXPECT(CVB(p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 5, 3, 1025, 0, 1.0f, 0, 0, p16, (size_t)1 << 40) == CRFP_E_UNSUPPORTED);
        EXPECT(CVB(p16, p16, p16, p16, p16, p16, p16, p16, p16, 70000, 5, 3, 7, 0, 1.0f, 0, 0, p16, (size_t)1 << 40) == CRFP_E_UNSUPPORTED);
        EXPECT(std::strstr(crfp_last_error_string(), "65535 images") != nullptr && std::strstr(crfp_last_error_string(), "2^58") != nullptr);
        EXPECT(CVB(p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 5, 3, 7, 2, 0.5f, 0, 0, p16, need - 1) == CRFP_E_WORKSPACE);
        EXPECT(CVB(p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 5, 3, 7, 2, 0.5f, 0, 0, nullptr, need) == CRFP_E_WORKSPACE);
        EXPECT(crfp_stub_launches() == l0);
        // gz always; weight transpose + input pass for grad_x / grad_x2; weight pass, bias pass and the slab sum as asked for
        EXPECT(CVB(p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 5, 3, 7, 2, 0.5f, 0, 0, p16, need) == 0 && crfp_stub_launches() == l0 + 6);
        EXPECT(CVB(nullptr, nullptr, p16, nullptr, p16, p16, nullptr, nullptr, nullptr, 2, 5, 3, 7, 0, 0.0f, 0, 0, p16, need) == 0 && crfp_stub_launches() == l0 + 9);
        EXPECT(CVB(nullptr, nullptr, p16, p16, p16, nullptr, p16, nullptr, nullptr, 2, 5, 3, 7, 4, -2.0f, 0, 0, p16, need) == 0 && crfp_stub_launches() == l0 + 12);
        EXPECT(CVB(p16, p16, nullptr, p16, p16, nullptr, nullptr, p16, nullptr, 2, 5, 3, 7, 2, 0.5f, 0, 0, p16, need) == 0 && crfp_stub_launches() == l0 + 15);
        EXPECT(CVB(nullptr, nullptr, nullptr, p16, p16, nullptr, nullptr, nullptr, p16, 2, 5, 3, 7, 2, 0.5f, 0, 0, p16, need) == 0 && crfp_stub_launches() == l0 + 18);
#undef CVB
        for (const auto& g : {std::initializer_list<int>{1, 32, 34, 32, 360, 640, 0, 0}, {1, 4, 4, 4, 1440, 2560, 0, 0}, {3, 128, 32, 288, 1, 1, 0, 0},
                              {2, 32, 0, 9, 5, 300, 4, 0}, {1, 8, 0, 32, 5, 6, 0, 4}, {1, 16, 0, 12, 7, 10, 0, 2}, {1, 1000, 24, 1024, 3, 70, 0, 0}}) {
            const int* v = g.begin();
            const size_t ws = crfp_conv3x3_ex_backward_workspace_bytes(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
            EXPECT(ws > 0 && crfp_conv3x3_ex_backward_f32(p16, v[1], p16, v[2], p16, p16, p16, p16, v[2] ? p16 : nullptr, p16, p16, v[0], v[3], v[4], v[5],
                                                          1, 1.0f, v[6], v[7], p16, ws, nullptr) == 0);
        }
        EXPECT(crfp_stub_launches() == l0 + 18 + 7 * 6);
    }
    // the resize / pool backward and the Charbonnier loss: every refusal before the first launch, then the launches a good call takes
    {
        const long l0 = crfp_stub_launches();
        EXPECT(crfp_upsample_bilinear_backward_f32(nullptr, p16, 1, 1, 2, 2, 4, 4, 0.5f, 0.5f, 1.0f, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_upsample_bilinear_backward_f32(p16, nullptr, 1, 1, 2, 2, 4, 4, 0.5f, 0.5f, 1.0f, nullptr) == CRFP_E_BADARG);
        const int bad_up[6][6] = {{0, 1, 2, 2, 4, 4}, {1, 0, 2, 2, 4, 4}, {1, 1, 0, 2, 4, 4}, {1, 1, 2, -1, 4, 4}, {1, 1, 2, 2, 0, 4}, {1, 1, 2, 2, 4, 0}};
        for (const auto& v : bad_up) EXPECT(crfp_upsample_bilinear_backward_f32(p16, p16, v[0], v[1], v[2], v[3], v[4], v[5], 0.5f, 0.5f, 1.0f, nullptr) == CRFP_E_BADARG);
        const float bad_scale[5] = {0.0f, -0.5f, NAN, INFINITY, -INFINITY};
        for (const float sc : bad_scale) {
            EXPECT(crfp_upsample_bilinear_backward_f32(p16, p16, 1, 1, 2, 2, 4, 4, sc, 0.5f, 1.0f, nullptr) == CRFP_E_BADARG);
            EXPECT(crfp_upsample_bilinear_backward_f32(p16, p16, 1, 1, 2, 2, 4, 4, 0.5f, sc, 1.0f, nullptr) == CRFP_E_BADARG);
        }
        EXPECT(std::strstr(crfp_last_error_string(), "positive and finite") != nullptr);
        EXPECT(crfp_upsample_bilinear_backward_f32(p16, p16, 65536, 1, 2, 2, 4, 4, 0.5f, 0.5f, 1.0f, nullptr) == CRFP_E_UNSUPPORTED);
        EXPECT(crfp_upsample_bilinear_backward_f32(p16, p16, 256, 256, 2, 2, 4, 4, 0.5f, 0.5f, 1.0f, nullptr) == CRFP_E_UNSUPPORTED);
        EXPECT(crfp_upsample_bilinear_backward_f32(p16, p16, 1, 1, 262141, 2, 4, 4, 0.5f, 0.5f, 1.0f, nullptr) == CRFP_E_UNSUPPORTED);
        EXPECT(crfp_upsample_bilinear_backward_f32(p16, p16, 1, 1, 2, (1 << 30) + 1, 4, 4, 0.5f, 0.5f, 1.0f, nullptr) == CRFP_E_UNSUPPORTED);
        EXPECT(crfp_upsample_bilinear_backward_f32(p16, p16, 65535, 1, 2, 2, 1 << 30, 1 << 30, 0.5f, 0.5f, 1.0f, nullptr) == CRFP_E_UNSUPPORTED);   // 2^58 elements
        EXPECT(crfp_avgpool2_backward_f32(nullptr, p16, 1, 1, 2, 2, nullptr) == CRFP_E_BADARG && crfp_avgpool2_backward_f32(p16, nullptr, 1, 1, 2, 2, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_avgpool2_backward_f32(p16, p16, 0, 1, 2, 2, nullptr) == CRFP_E_BADARG && crfp_avgpool2_backward_f32(p16, p16, 1, 0, 2, 2, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_avgpool2_backward_f32(p16, p16, 1, 1, 1, 2, nullptr) == CRFP_E_BADARG && crfp_avgpool2_backward_f32(p16, p16, 1, 1, 2, 1, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_avgpool2_backward_f32(p16, p16, 65536, 1, 2, 2, nullptr) == CRFP_E_UNSUPPORTED && crfp_avgpool2_backward_f32(p16, p16, 1, 1, 300000, 2, nullptr) == CRFP_E_UNSUPPORTED);
        const size_t need = crfp_charbonnier_workspace_bytes(2, 3, 9, 11);
        EXPECT(need >= 2 * 2 * sizeof(double) && crfp_charbonnier_workspace_bytes(1, 3, 1440, 2560) >= need);
        EXPECT(crfp_charbonnier_workspace_bytes(0, 3, 9, 11) == 0 && crfp_charbonnier_workspace_bytes(2, 0, 9, 11) == 0 && crfp_charbonnier_workspace_bytes(2, 3, -1, 11) == 0);
        EXPECT(crfp_charbonnier_workspace_bytes(2, 3, 9, 0) == 0 && crfp_charbonnier_workspace_bytes(65536, 3, 9, 11) == 0);
        EXPECT(crfp_charbonnier_workspace_bytes(65535, 2147483647, 2147483647, 2147483647) == 0);
        double* const d16 = reinterpret_cast<double*>(p16);
#define CBF(P, T, W, WC, S, N, C, EPS, WS, WSB) crfp_charbonnier_f32(P, T, W, WC, S, N, C, 9, 11, EPS, WS, WSB, nullptr)
#define CBB(P, T, W, WC, SC, G, N, C, EPS) crfp_charbonnier_backward_f32(P, T, W, WC, SC, G, N, C, 9, 11, EPS, nullptr)
        EXPECT(CBF(nullptr, p16, nullptr, 0, d16, 2, 3, 1e-12f, p16, need) == CRFP_E_BADARG && CBF(p16, nullptr, nullptr, 0, d16, 2, 3, 1e-12f, p16, need) == CRFP_E_BADARG);
        EXPECT(CBF(p16, p16, nullptr, 0, nullptr, 2, 3, 1e-12f, p16, need) == CRFP_E_BADARG && std::strstr(crfp_last_error_string(), "null") != nullptr);
        EXPECT(CBF(p16, p16, nullptr, 0, d16, 0, 3, 1e-12f, p16, need) == CRFP_E_BADARG && CBF(p16, p16, nullptr, 0, d16, 2, 0, 1e-12f, p16, need) == CRFP_E_BADARG);
        EXPECT(CBF(p16, p16, nullptr, 1, d16, 2, 3, 1e-12f, p16, need) == CRFP_E_BADARG && CBF(p16, p16, p16, 0, d16, 2, 3, 1e-12f, p16, need) == CRFP_E_BADARG);
        EXPECT(CBF(p16, p16, p16, 2, d16, 2, 3, 1e-12f, p16, need) == CRFP_E_BADARG && std::strstr(crfp_last_error_string(), "weight_c") != nullptr);
        EXPECT(CBF(p16, p16, nullptr, 0, d16, 2, 3, -1.0f, p16, need) == CRFP_E_BADARG && CBF(p16, p16, nullptr, 0, d16, 2, 3, NAN, p16, need) == CRFP_E_BADARG);
        EXPECT(CBF(p16, p16, nullptr, 0, d16, 65536, 3, 1e-12f, p16, (size_t)1 << 40) == CRFP_E_UNSUPPORTED);
        EXPECT(CBF(p16, p16, nullptr, 0, d16, 2, 3, 1e-12f, nullptr, need) == CRFP_E_WORKSPACE && CBF(p16, p16, nullptr, 0, d16, 2, 3, 1e-12f, p16, need - 1) == CRFP_E_WORKSPACE);
        EXPECT(CBB(nullptr, p16, nullptr, 0, p16, p16, 2, 3, 1e-12f) == CRFP_E_BADARG && CBB(p16, nullptr, nullptr, 0, p16, p16, 2, 3, 1e-12f) == CRFP_E_BADARG);
        EXPECT(CBB(p16, p16, nullptr, 0, nullptr, p16, 2, 3, 1e-12f) == CRFP_E_BADARG && CBB(p16, p16, nullptr, 0, p16, nullptr, 2, 3, 1e-12f) == CRFP_E_BADARG);
        EXPECT(CBB(p16, p16, nullptr, 3, p16, p16, 2, 3, 1e-12f) == CRFP_E_BADARG && CBB(p16, p16, p16, 2, p16, p16, 2, 3, 1e-12f) == CRFP_E_BADARG);
        EXPECT(CBB(p16, p16, nullptr, 0, p16, p16, 2, 3, INFINITY) == CRFP_E_BADARG && CBB(p16, p16, nullptr, 0, p16, p16, 70000, 3, 1e-12f) == CRFP_E_UNSUPPORTED);
        EXPECT(crfp_stub_launches() == l0);
        EXPECT(crfp_upsample_bilinear_backward_f32(p16, p16, 2, 3, 5, 7, 40, 56, 0.125f, 0.125f, 8.0f, nullptr) == 0 && crfp_stub_launches() == l0 + 1);
        EXPECT(crfp_upsample_bilinear_backward_f32(p16, p16, 1, 1, 262140, 1, 1, 1 << 30, 1e-30f, 3e38f, 1.0f, nullptr) == 0 && crfp_stub_launches() == l0 + 2);
        EXPECT(crfp_avgpool2_backward_f32(p16, p16, 2, 3, 45, 80, nullptr) == 0 && crfp_stub_launches() == l0 + 3);
        EXPECT(CBF(p16, p16, nullptr, 0, d16, 2, 3, 1e-12f, p16, need) == 0 && crfp_stub_launches() == l0 + 5);   // partials, then the fixed-order sum
        EXPECT(CBF(p16, p16, p16, 1, d16, 2, 3, 0.0f, p16, need) == 0 && CBF(p16, p16, p16, 3, d16, 2, 3, 1e-6f, p16, need) == 0 && crfp_stub_launches() == l0 + 9);
        EXPECT(CBB(p16, p16, nullptr, 0, p16, p16, 2, 3, 1e-12f) == 0 && CBB(p16, p16, p16, 1, p16, p16, 2, 3, 1e-12f) == 0 && crfp_stub_launches() == l0 + 11);
        EXPECT(crfp_charbonnier_f32(p16, p16, nullptr, 0, d16, 8, 3, 4320, 7680, 1e-12f, p16, crfp_charbonnier_workspace_bytes(8, 3, 4320, 7680), nullptr) == 0);
#undef CBF
#undef CBB
    }
    // the DCNv2 backward: sizing, every refusal before the first launch, the launches each subset of wanted outputs takes
    {
        const size_t need = crfp_dcnv2_backward_workspace_bytes(2, 8, 6, 9, 11, 3, 2);
        EXPECT(need > 0 && crfp_dcnv2_backward_workspace_bytes(1, 32, 32, 360, 640, 3, 8) > 0 && crfp_dcnv2_backward_workspace_bytes(1, 4, 4, 1440, 2560, 3, 1) > 0);
        EXPECT(crfp_dcnv2_backward_workspace_bytes(1, 64, 64, 8, 8, 3, 64) > crfp_dcnv2_backward_workspace_bytes(1, 64, 32, 8, 8, 3, 64));
        EXPECT(crfp_dcnv2_backward_workspace_bytes(0, 8, 6, 9, 11, 3, 2) == 0 && crfp_dcnv2_backward_workspace_bytes(2, 8, 6, 9, 11, 5, 2) == 0);
        EXPECT(crfp_dcnv2_backward_workspace_bytes(2, 8, 6, 9, 11, 3, 3) == 0 && crfp_dcnv2_backward_workspace_bytes(2, 65, 6, 9, 11, 3, 1) == 0);
        EXPECT(crfp_dcnv2_backward_workspace_bytes(2, 8, 66, 9, 11, 3, 2) == 0 && crfp_dcnv2_backward_workspace_bytes(2, 8, 6, 9, 11, 3, 0) == 0);
        EXPECT(crfp_dcnv2_backward_workspace_bytes(70000, 8, 6, 9, 11, 3, 2) == 0 && crfp_dcnv2_backward_workspace_bytes(1, 8, 6, 300000, 1, 3, 2) == 0);
        EXPECT(crfp_dcnv2_backward_workspace_bytes(65535, 64, 64, 262140, 2147483647, 3, 1) == 0);   // element counts beyond 64-bit indexing
        EXPECT(crfp_dcnv2_backward_workspace_bytes(8, 64, 64, 4320, 7680, 3, 8) > 0 && crfp_dcnv2_backward_workspace_bytes(1, 1, 1, 262140, 100000, 3, 1) > 0);
        const long l0 = crfp_stub_launches();
#define DCNB(X, OFF, M, W, GO, GX, GOFF, GM, GW, GB, N, CIN, COUT, K, PAD, DIL, DG, WS, WSB) \
    crfp_dcnv2_backward_f32(X, OFF, M, W, GO, GX, GOFF, GM, GW, GB, N, CIN, COUT, 9, 11, K, PAD, DIL, DG, WS, WSB, nullptr)
        EXPECT(DCNB(nullptr, p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 8, 6, 3, 1, 1, 2, p16, need) == CRFP_E_BADARG);
        EXPECT(std::strstr(crfp_last_error_string(), "null") != nullptr);
        EXPECT(DCNB(p16, nullptr, p16, p16, p16, p16, p16, p16, p16, p16, 2, 8, 6, 3, 1, 1, 2, p16, need) == CRFP_E_BADARG);
        EXPECT(DCNB(p16, p16, nullptr, p16, p16, p16, p16, p16, p16, p16, 2, 8, 6, 3, 1, 1, 2, p16, need) == CRFP_E_BADARG);
        EXPECT(DCNB(p16, p16, p16, nullptr, p16, p16, p16, p16, p16, p16, 2, 8, 6, 3, 1, 1, 2, p16, need) == CRFP_E_BADARG);
        EXPECT(DCNB(p16, p16, p16, p16, nullptr, p16, p16, p16, p16, p16, 2, 8, 6, 3, 1, 1, 2, p16, need) == CRFP_E_BADARG);
        EXPECT(DCNB(p16, p16, p16, p16, p16, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 8, 6, 3, 1, 1, 2, p16, need) == CRFP_E_BADARG);
        EXPECT(std::strstr(crfp_last_error_string(), "nothing to do") != nullptr);
        EXPECT(DCNB(p16, p16, p16, p16, p16, p16, p16, p16, p16, p16, 0, 8, 6, 3, 1, 1, 2, p16, need) == CRFP_E_BADARG);
        EXPECT(DCNB(p16, p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 8, 6, 3, 1, 1, 0, p16, need) == CRFP_E_BADARG);
        EXPECT(DCNB(p16, p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 8, 6, 5, 2, 1, 2, p16, need) == CRFP_E_UNSUPPORTED);
        EXPECT(std::strstr(crfp_last_error_string(), "kernel 3") != nullptr);
        EXPECT(DCNB(p16, p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 8, 6, 3, 0, 1, 2, p16, need) == CRFP_E_UNSUPPORTED);
        EXPECT(DCNB(p16, p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 8, 6, 3, 1, 2, 2, p16, need) == CRFP_E_UNSUPPORTED);
        EXPECT(DCNB(p16, p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 8, 6, 3, 1, 1, 3, p16, need) == CRFP_E_UNSUPPORTED);
        EXPECT(std::strstr(crfp_last_error_string(), "deformable_groups") != nullptr);
        EXPECT(DCNB(p16, p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 65, 6, 3, 1, 1, 1, p16, (size_t)1 << 40) == CRFP_E_UNSUPPORTED);
        EXPECT(DCNB(p16, p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 8, 128, 3, 1, 1, 2, p16, (size_t)1 << 40) == CRFP_E_UNSUPPORTED);
        EXPECT(DCNB(p16, p16, p16, p16, p16, p16, p16, p16, p16, p16, 70000, 8, 6, 3, 1, 1, 2, p16, (size_t)1 << 40) == CRFP_E_UNSUPPORTED);
        EXPECT(DCNB(p16, p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 8, 6, 3, 1, 1, 2, p16, need - 1) == CRFP_E_WORKSPACE);
        EXPECT(DCNB(p16, p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 8, 6, 3, 1, 1, 2, nullptr, need) == CRFP_E_WORKSPACE);
        EXPECT(crfp_stub_launches() == l0);
        // weight transpose + pixel kernel when grad_x, grad_offset or grad_mask is wanted; slab pass + slab sum when grad_weight or grad_bias is
        EXPECT(DCNB(p16, p16, p16, p16, p16, p16, p16, p16, p16, p16, 2, 8, 6, 3, 1, 1, 2, p16, need) == 0 && crfp_stub_launches() == l0 + 4);
        EXPECT(DCNB(p16, p16, p16, p16, p16, p16, nullptr, nullptr, nullptr, nullptr, 2, 8, 6, 3, 1, 1, 2, p16, need) == 0 && crfp_stub_launches() == l0 + 6);
        EXPECT(DCNB(p16, p16, p16, p16, p16, nullptr, p16, p16, nullptr, nullptr, 2, 8, 6, 3, 1, 1, 2, p16, need) == 0 && crfp_stub_launches() == l0 + 8);
        EXPECT(DCNB(p16, p16, p16, p16, p16, nullptr, nullptr, nullptr, p16, nullptr, 2, 8, 6, 3, 1, 1, 2, p16, need) == 0 && crfp_stub_launches() == l0 + 10);
        EXPECT(DCNB(p16, p16, p16, p16, p16, nullptr, nullptr, nullptr, nullptr, p16, 2, 8, 6, 3, 1, 1, 2, p16, need) == 0 && crfp_stub_launches() == l0 + 12);
#undef DCNB
        for (const auto& g : {std::initializer_list<int>{1, 32, 32, 8, 360, 640}, {1, 4, 4, 1, 1440, 2560}, {3, 64, 64, 64, 1, 1}, {2, 33, 7, 11, 5, 300}}) {
            const int n = g.begin()[0], ci = g.begin()[1], co = g.begin()[2], dg = g.begin()[3], h = g.begin()[4], w = g.begin()[5];
            const size_t ws = crfp_dcnv2_backward_workspace_bytes(n, ci, co, h, w, 3, dg);
            EXPECT(ws > 0 && crfp_dcnv2_backward_f32(p16, p16, p16, p16, p16, p16, p16, p16, p16, p16, n, ci, co, h, w, 3, 1, 1, dg, p16, ws, nullptr) == 0);
        }
        EXPECT(crfp_stub_launches() == l0 + 12 + 4 * 4);
    }
    // the shared-offset DCNv2 backward: the 4 -> 4 domain, the compact route's scratch (no tiled tensor), refusals before the first launch
    {
        const size_t need = crfp_dcnv2_shared_backward_workspace_bytes(1, 4, 24, 40);
        EXPECT(need > 0 && need == crfp_dcnv2_backward_workspace_bytes(1, 4, 4, 24, 40, 3, 1));
        const size_t big = crfp_dcnv2_shared_backward_workspace_bytes(1, 4, 1440, 2560);
        EXPECT(big > 0 && big < (1u << 20));   // weight transpose + per-workgroup slabs: nowhere near 27 planes of 1440 x 2560
        EXPECT(crfp_dcnv2_shared_backward_workspace_bytes(1, 8, 24, 40) == 0 && crfp_dcnv2_shared_backward_workspace_bytes(1, 3, 24, 40) == 0);
        EXPECT(crfp_dcnv2_shared_backward_workspace_bytes(0, 4, 24, 40) == 0 && crfp_dcnv2_shared_backward_workspace_bytes(1, 4, 0, 40) == 0);
        EXPECT(crfp_dcnv2_shared_backward_workspace_bytes(70000, 4, 24, 40) == 0 && crfp_dcnv2_shared_backward_workspace_bytes(1, 4, 300000, 40) == 0);
        EXPECT(crfp_dcnv2_shared_backward_workspace_bytes(65535, 4, 262140, 2147483647) == 0);
        const long l0 = crfp_stub_launches();
#define DCNS(X, OFF, M, W, GO, GX, GOFF, GM, GW, GB, N, CIN, COUT, WS, WSB) \
    crfp_dcnv2_shared_backward_f32(X, OFF, M, W, GO, GX, GOFF, GM, GW, GB, N, CIN, COUT, 24, 40, WS, WSB, nullptr)
        EXPECT(DCNS(nullptr, p16, p16, p16, p16, p16, p16, p16, p16, p16, 1, 4, 4, p16, need) == CRFP_E_BADARG);
        EXPECT(std::strstr(crfp_last_error_string(), "null") != nullptr);
        EXPECT(DCNS(p16, nullptr, p16, p16, p16, p16, p16, p16, p16, p16, 1, 4, 4, p16, need) == CRFP_E_BADARG);
        EXPECT(DCNS(p16, p16, nullptr, p16, p16, p16, p16, p16, p16, p16, 1, 4, 4, p16, need) == CRFP_E_BADARG);
        EXPECT(DCNS(p16, p16, p16, nullptr, p16, p16, p16, p16, p16, p16, 1, 4, 4, p16, need) == CRFP_E_BADARG);
        EXPECT(DCNS(p16, p16, p16, p16, nullptr, p16, p16, p16, p16, p16, 1, 4, 4, p16, need) == CRFP_E_BADARG);
        EXPECT(DCNS(p16, p16, p16, p16, p16, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 4, 4, p16, need) == CRFP_E_BADARG);
        EXPECT(std::strstr(crfp_last_error_string(), "nothing to do") != nullptr);
        EXPECT(DCNS(p16, p16, p16, p16, p16, p16, p16, p16, p16, p16, 0, 4, 4, p16, need) == CRFP_E_BADARG);
        EXPECT(DCNS(p16, p16, p16, p16, p16, p16, p16, p16, p16, p16, 1, 8, 4, p16, (size_t)1 << 40) == CRFP_E_UNSUPPORTED);
        EXPECT(std::strstr(crfp_last_error_string(), "4 -> 4") != nullptr);
        EXPECT(DCNS(p16, p16, p16, p16, p16, p16, p16, p16, p16, p16, 1, 4, 8, p16, (size_t)1 << 40) == CRFP_E_UNSUPPORTED);
        EXPECT(DCNS(p16, p16, p16, p16, p16, p16, p16, p16, p16, p16, 70000, 4, 4, p16, (size_t)1 << 40) == CRFP_E_UNSUPPORTED);
        EXPECT(std::strstr(crfp_last_error_string(), "65535 images") != nullptr);
        EXPECT(DCNS(p16, p16, p16, p16, p16, p16, p16, p16, p16, p16, 1, 4, 4, p16, need - 1) == CRFP_E_WORKSPACE);
        EXPECT(DCNS(p16, p16, p16, p16, p16, p16, p16, p16, p16, p16, 1, 4, 4, nullptr, need) == CRFP_E_WORKSPACE);
        EXPECT(crfp_stub_launches() == l0);
        // the launches of crfp_dcnv2_backward_f32: transpose + pixel kernel for grad_x / grad_offset / grad_mask, slab pass + slab sum for the rest
        EXPECT(DCNS(p16, p16, p16, p16, p16, p16, p16, p16, p16, p16, 1, 4, 4, p16, need) == 0 && crfp_stub_launches() == l0 + 4);
        EXPECT(DCNS(p16, p16, p16, p16, p16, p16, nullptr, nullptr, nullptr, nullptr, 1, 4, 4, p16, need) == 0 && crfp_stub_launches() == l0 + 6);
        EXPECT(DCNS(p16, p16, p16, p16, p16, nullptr, p16, p16, nullptr, nullptr, 1, 4, 4, p16, need) == 0 && crfp_stub_launches() == l0 + 8);
        EXPECT(DCNS(p16, p16, p16, p16, p16, nullptr, nullptr, nullptr, nullptr, p16, 1, 4, 4, p16, need) == 0 && crfp_stub_launches() == l0 + 10);
#undef DCNS
        EXPECT(crfp_dcnv2_shared_backward_f32(p16, p16, p16, p16, p16, p16, p16, p16, p16, p16, 1, 4, 4, 1440, 2560, p16, big, nullptr) == 0);
        EXPECT(crfp_stub_launches() == l0 + 14);
    }
    // the flow_warp backward: sizing, the NULL-output rules, every refusal before the first launch, one launch per accepted call
    {
        const size_t need = crfp_flow_warp_backward_workspace_bytes(2, 5, 9, 11);
        EXPECT(need > 0 && crfp_flow_warp_backward_workspace_bytes(1, 32, 360, 640) > 0 && crfp_flow_warp_backward_workspace_bytes(1, 4, 1440, 2560) > 0);
        EXPECT(crfp_flow_warp_backward_workspace_bytes(1, 3, 1, 7) > 0 && crfp_flow_warp_backward_workspace_bytes(1, 3, 6, 1) > 0);
        EXPECT(crfp_flow_warp_backward_workspace_bytes(0, 5, 9, 11) == 0 && crfp_flow_warp_backward_workspace_bytes(2, 0, 9, 11) == 0);
        EXPECT(crfp_flow_warp_backward_workspace_bytes(2, 5, 0, 11) == 0 && crfp_flow_warp_backward_workspace_bytes(2, 5, 9, 0) == 0);
        EXPECT(crfp_flow_warp_backward_workspace_bytes(70000, 5, 9, 11) == 0 && crfp_flow_warp_backward_workspace_bytes(2, 5, 300000, 11) == 0);
        EXPECT(crfp_flow_warp_backward_workspace_bytes(2, 5, 9, (1 << 30) + 1) == 0);
        EXPECT(crfp_flow_warp_backward_workspace_bytes(65535, 1 << 20, 262140, 1 << 30) == 0);   // element counts beyond 64-bit indexing
        EXPECT(crfp_flow_warp_backward_workspace_bytes(8, 64, 4320, 7680) > 0 && crfp_flow_warp_backward_workspace_bytes(1, 1, 262140, 100000) > 0);
        const long l0 = crfp_stub_launches();
#define WARPB(X, FLOW, GO, GX, GFLOW, N, C, MODE, WS, WSB) crfp_flow_warp_backward_f32(X, FLOW, GO, GX, GFLOW, N, C, 9, 11, MODE, WS, WSB, nullptr)
        EXPECT(WARPB(p16, p16, p16, nullptr, nullptr, 2, 5, CRFP_PAD_ZEROS, p16, need) == CRFP_E_BADARG);
        EXPECT(std::strstr(crfp_last_error_string(), "nothing to do") != nullptr);
        EXPECT(WARPB(nullptr, p16, p16, p16, p16, 2, 5, CRFP_PAD_ZEROS, p16, need) == CRFP_E_BADARG);
        EXPECT(std::strstr(crfp_last_error_string(), "grad_flow") != nullptr);
        EXPECT(WARPB(nullptr, p16, p16, nullptr, p16, 2, 5, CRFP_PAD_BORDER, p16, need) == CRFP_E_BADARG);
        EXPECT(WARPB(p16, nullptr, p16, p16, p16, 2, 5, CRFP_PAD_ZEROS, p16, need) == CRFP_E_BADARG);
        EXPECT(WARPB(p16, p16, nullptr, p16, p16, 2, 5, CRFP_PAD_ZEROS, p16, need) == CRFP_E_BADARG);
        EXPECT(WARPB(p16, p16, p16, p16, p16, 0, 5, CRFP_PAD_ZEROS, p16, need) == CRFP_E_BADARG);
        EXPECT(WARPB(p16, p16, p16, p16, p16, 2, 0, CRFP_PAD_ZEROS, p16, need) == CRFP_E_BADARG);
        EXPECT(WARPB(p16, p16, p16, p16, p16, 2, 5, 2, p16, need) == CRFP_E_UNSUPPORTED);
        EXPECT(std::strstr(crfp_last_error_string(), "padding_mode") != nullptr);
        EXPECT(WARPB(p16, p16, p16, p16, p16, 2, 5, -1, p16, need) == CRFP_E_UNSUPPORTED);
        EXPECT(WARPB(p16, p16, p16, p16, p16, 70000, 5, CRFP_PAD_ZEROS, p16, (size_t)1 << 40) == CRFP_E_UNSUPPORTED);
        EXPECT(std::strstr(crfp_last_error_string(), "2^58") != nullptr);
        EXPECT(WARPB(p16, p16, p16, p16, p16, 2, 5, CRFP_PAD_ZEROS, p16, need - 1) == CRFP_E_WORKSPACE);
        EXPECT(WARPB(p16, p16, p16, p16, p16, 2, 5, CRFP_PAD_BORDER, nullptr, need) == CRFP_E_WORKSPACE);
        EXPECT(crfp_flow_warp_backward_window_f32(p16, p16, p16, p16, p16, 2, 5, 9, 11, CRFP_PAD_ZEROS, 2, p16, need, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_stub_launches() == l0);
        EXPECT(WARPB(p16, p16, p16, p16, p16, 2, 5, CRFP_PAD_ZEROS, p16, need) == 0 && crfp_stub_launches() == l0 + 1);
        EXPECT(WARPB(p16, p16, p16, p16, p16, 2, 5, CRFP_PAD_BORDER, p16, need) == 0 && crfp_stub_launches() == l0 + 2);
        EXPECT(WARPB(nullptr, p16, p16, p16, nullptr, 2, 5, CRFP_PAD_ZEROS, p16, need) == 0 && crfp_stub_launches() == l0 + 3);   // x is read for grad_flow only
        EXPECT(WARPB(p16, p16, p16, nullptr, p16, 2, 5, CRFP_PAD_BORDER, p16, need) == 0 && crfp_stub_launches() == l0 + 4);
#undef WARPB
        EXPECT(crfp_flow_warp_backward_window_f32(p16, p16, p16, p16, p16, 1, 32, 360, 640, CRFP_PAD_ZEROS, 0, p16, need, nullptr) == 0);
        EXPECT(crfp_flow_warp_backward_f32(p16, p16, p16, p16, p16, 1, 4, 1440, 2560, CRFP_PAD_BORDER, p16, need, nullptr) == 0);
        EXPECT(crfp_stub_launches() == l0 + 6);
    }
    // the conv probe (test hook): sizing, the launcher's kernel-selection rule, every refusal before the first launch, whole calls on the stub
    {
        crfp_probe_conv q;
        std::memset(&q, 0, sizeof(q));
        q.nsrc = 1; q.src_kind[0] = CRFP_PROBE_SRC_Q4; q.src_nch[0] = 32; q.cout = 32; q.store = CRFP_PROBE_ST_Q4; q.post_scale = 1.0f;
        q.ndst = 1; q.dst_q1[0] = 8;
        int k[2] = {-1, -1};
        const long l0 = crfp_stub_launches();
        const size_t w32 = crfp_conv_probe_workspace_bytes(CRFP_PROBE_SINGLE, &q, nullptr, 3, 9, 130);
        const size_t w16 = crfp_conv_probe_workspace_bytes_bf16(CRFP_PROBE_SINGLE, &q, nullptr, 3, 9, 130);
        EXPECT(w32 > 2ull * 3 * 8 * 9 * 130 * 16 && w16 > 0 && w16 < w32);
        // selection: one cout tile -> the 8-wave kernels; the bf16 build's 512-slot rule on both sides; two tiles -> the 4-wave kernels
        EXPECT(crfp_conv_probe_kernel(CRFP_PROBE_SINGLE, &q, nullptr, 19, 72, 192, k) == 0 && k[0] == CRFP_CONVK_SPLIT8 && k[1] == CRFP_CONVK_NONE);
        EXPECT(crfp_conv_probe_kernel_bf16(CRFP_PROBE_SINGLE, &q, nullptr, 19, 72, 192, k) == 0 && k[0] == CRFP_CONVK_BF16_4W);
        EXPECT(crfp_conv_probe_kernel_bf16(CRFP_PROBE_SINGLE, &q, nullptr, 16, 64, 256, k) == 0 && k[0] == CRFP_CONVK_BF16_X8);
        EXPECT(crfp_conv_probe_kernel_bf16(CRFP_PROBE_SINGLE, &q, nullptr, 1, 72, 192, k) == 0 && k[0] == CRFP_CONVK_BF16_X8);
        crfp_probe_conv s = q;
        s.strict = 1;
        EXPECT(crfp_conv_probe_kernel(CRFP_PROBE_SINGLE, &s, nullptr, 1, 72, 192, k) == 0 && k[0] == CRFP_CONVK_MFMA_ROWS4);
        EXPECT(crfp_conv_probe_kernel(CRFP_PROBE_SINGLE, &s, nullptr, 19, 72, 192, k) == 0 && k[0] == CRFP_CONVK_MFMA_ROWS8);
        crfp_probe_conv big = q;
        big.src_nch[0] = 324;   // over the per-quad descriptor table: fp32 MFMA
        EXPECT(crfp_conv_probe_kernel(CRFP_PROBE_SINGLE, &big, nullptr, 1, 4, 64, k) == 0 && k[0] == CRFP_CONVK_MFMA_ROWS4);
        crfp_probe_conv two = q;
        two.cout = 64; two.dst_q1[0] = 16;
        EXPECT(crfp_conv_probe_kernel(CRFP_PROBE_SINGLE, &two, nullptr, 2, 8, 65, k) == 0 && k[0] == CRFP_CONVK_SPLIT4);
        EXPECT(crfp_conv_probe_kernel_bf16(CRFP_PROBE_SINGLE, &two, nullptr, 2, 8, 65, k) == 0 && k[0] == CRFP_CONVK_BF16_4W);
        EXPECT(crfp_conv_probe_kernel(CRFP_PROBE_SINGLE, &s, nullptr, 1, 72, 192, nullptr) == CRFP_E_BADARG);
        s = two; s.strict = 1;
        EXPECT(crfp_conv_probe_kernel(CRFP_PROBE_SINGLE, &s, nullptr, 2, 8, 65, k) == 0 && k[0] == CRFP_CONVK_MFMA_CT2);
        // dual: 4-row tiles * cout tiles a multiple of 8 or not
        EXPECT(crfp_conv_probe_kernel(CRFP_PROBE_DUAL, &two, &two, 2, 8, 65, k) == 0 && k[0] == CRFP_CONVK_SPLIT_DUAL && k[1] == CRFP_CONVK_SPLIT_DUAL);
        EXPECT(crfp_conv_probe_kernel(CRFP_PROBE_DUAL, &two, &two, 2, 9, 64, k) == 0 && k[0] == CRFP_CONVK_SPLIT4 && k[1] == CRFP_CONVK_SPLIT4);
        EXPECT(crfp_conv_probe_kernel(CRFP_PROBE_DUAL, &two, &q, 2, 8, 65, k) == 0 && k[0] == CRFP_CONVK_SPLIT4 && k[1] == CRFP_CONVK_SPLIT8);
        EXPECT(crfp_conv_probe_kernel_bf16(CRFP_PROBE_DUAL, &two, &two, 2, 8, 65, k) == 0 && k[0] == CRFP_CONVK_BF16_4W);
        // pair / S3 chain: each in its own build only
        crfp_probe_conv a0 = q;
        a0.ndst = 0;
        EXPECT(crfp_conv_probe_kernel(CRFP_PROBE_PAIR, &a0, &q, 2, 8, 62, k) == CRFP_E_UNSUPPORTED);
        EXPECT(crfp_conv_probe_kernel_bf16(CRFP_PROBE_PAIR, &a0, &q, 2, 8, 62, k) == 0 && k[0] == CRFP_CONVK_BF16_PAIR && k[1] == CRFP_CONVK_BF16_PAIR);
        EXPECT(crfp_conv_probe_kernel(CRFP_PROBE_PAIR_F32, &a0, &q, 2, 8, 62, k) == 0 && k[0] == CRFP_CONVK_SPLIT_PAIR && k[1] == CRFP_CONVK_SPLIT_PAIR);
        EXPECT(crfp_conv_probe_kernel_bf16(CRFP_PROBE_PAIR_F32, &a0, &q, 2, 8, 62, k) == CRFP_E_UNSUPPORTED);
        EXPECT(crfp_conv_probe_kernel(CRFP_PROBE_PAIR_F32 + 1, &a0, &q, 2, 8, 62, k) == CRFP_E_BADARG);
        EXPECT(crfp_conv_probe_workspace_bytes(CRFP_PROBE_PAIR_F32, &a0, &q, 2, 8, 62) > 0 && crfp_conv_probe_workspace_bytes_bf16(CRFP_PROBE_PAIR_F32, &a0, &q, 2, 8, 62) == 0);
        EXPECT(crfp_conv_probe_kernel_bf16(CRFP_PROBE_S3_CHAIN, &a0, &two, 2, 8, 62, k) == CRFP_E_UNSUPPORTED);
        EXPECT(crfp_conv_probe_kernel(CRFP_PROBE_S3_CHAIN, &a0, &two, 2, 8, 62, k) == 0 && k[0] == CRFP_CONVK_SPLIT8 && k[1] == CRFP_CONVK_SPLIT4);
        EXPECT(crfp_conv_probe_workspace_bytes(CRFP_PROBE_S3_CHAIN, &a0, &two, 2, 8, 62) > 0);
        // refusals of the sizing function
        EXPECT(crfp_conv_probe_workspace_bytes(CRFP_PROBE_SINGLE, &a0, nullptr, 2, 8, 62) == 0);     // no destination
        EXPECT(std::strstr(crfp_last_error_string(), "destinations") != nullptr);
        EXPECT(crfp_conv_probe_workspace_bytes(CRFP_PROBE_SINGLE, nullptr, nullptr, 2, 8, 62) == 0);
        EXPECT(crfp_conv_probe_workspace_bytes(CRFP_PROBE_DUAL, &q, nullptr, 2, 8, 62) == 0);
        EXPECT(crfp_conv_probe_workspace_bytes(4, &q, nullptr, 2, 8, 62) == 0 && crfp_conv_probe_workspace_bytes(-1, &q, nullptr, 2, 8, 62) == 0);
        EXPECT(crfp_conv_probe_workspace_bytes(CRFP_PROBE_SINGLE, &q, nullptr, 0, 8, 62) == 0);
        EXPECT(crfp_conv_probe_workspace_bytes(CRFP_PROBE_SINGLE, &q, nullptr, 2, 8, 0) == 0);
        EXPECT(crfp_conv_probe_workspace_bytes(CRFP_PROBE_SINGLE, &q, nullptr, 70000, 8, 62) == 0);
        for (int f = 0; f < 10; ++f) {
            crfp_probe_conv d = q;
            switch (f) {
                case 0: d.nsrc = 5; break;
                case 1: d.src_kind[0] = 1; break;                              // NCHW sources are not the probe's
                case 2: d.src_kind[0] = CRFP_PROBE_SRC_UNSHUF4; d.src_nch[0] = 24; break;
                case 3: d.src_kind[0] = CRFP_PROBE_SRC_FLOW2; d.src_nch[0] = 3; break;
                case 4: d.src_pad[0] = 2; break;
                case 5: d.cout = 0; break;
                case 6: d.act = 9; break;
                case 7: d.dst_q1[0] = 9; break;
                case 8: d.store = CRFP_PROBE_ST_PS; d.ps_r = 3; break;
                default: d.store = CRFP_PROBE_ST_OFFMASK; d.n_off_quads = 9; break;
            }
            EXPECT(crfp_conv_probe_workspace_bytes(CRFP_PROBE_SINGLE, &d, nullptr, 2, 8, 62) == 0);
            EXPECT(crfp_conv_probe_workspace_bytes_bf16(CRFP_PROBE_SINGLE, &d, nullptr, 2, 8, 62) == 0);
        }
        // the call: null tensors, null status / kernel, a short workspace -- all before the first launch
        unsigned* const st = reinterpret_cast<unsigned*>(16);
        EXPECT(crfp_conv_probe(CRFP_PROBE_SINGLE, &q, nullptr, 3, 9, 130, st, k, p16, w32, nullptr) == CRFP_E_BADARG);   // null tensors
        q.src[0] = p16; q.weight = p16; q.bias = p16; q.dst[0] = p16;
        EXPECT(crfp_conv_probe(CRFP_PROBE_SINGLE, &q, nullptr, 3, 9, 130, nullptr, k, p16, w32, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_conv_probe(CRFP_PROBE_SINGLE, &q, nullptr, 3, 9, 130, st, nullptr, p16, w32, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_conv_probe(CRFP_PROBE_SINGLE, &q, nullptr, 3, 9, 130, st, k, p16, w32 - 1, nullptr) == CRFP_E_WORKSPACE);
        EXPECT(crfp_conv_probe(CRFP_PROBE_SINGLE, &q, nullptr, 3, 9, 130, st, k, nullptr, w32, nullptr) == CRFP_E_WORKSPACE);
        EXPECT(crfp_stub_launches() == l0);
        // accepted calls on the stub runtime, device pointers fabricated: every mode, both builds, ragged and padded plans
        char* const dev = reinterpret_cast<char*>(0x200000000000ull);
        auto fab = [&](crfp_probe_conv& d, int slot) {
            float* const base = reinterpret_cast<float*>(dev + ((size_t)slot << 32));
            for (int i = 0; i < CRFP_PROBE_MAX_SRC; ++i) d.src[i] = base + (i << 24);
            d.weight = base + (5 << 24); d.bias = base + (6 << 24); d.weight2 = base + (7 << 24); d.bias2 = base + (8 << 24);
            d.flow = base + (9 << 24);
            for (int i = 0; i < CRFP_PROBE_MAX_DST; ++i) { d.dst[i] = base + ((10 + i) << 24); d.dst_raw[i] = base + ((13 + i) << 24); }
        };
        crfp_probe_conv m = q;
        m.nsrc = 4; m.src_nch[0] = 24; m.src_pad[0] = 1; m.src_kind[1] = CRFP_PROBE_SRC_Q4; m.src_nch[1] = 8;
        m.src_kind[2] = CRFP_PROBE_SRC_UNSHUF4; m.src_nch[2] = 64; m.src_kind[3] = CRFP_PROBE_SRC_FLOW2; m.src_nch[3] = 2;
        m.cout = 38; m.ndst = 3; m.dst_q0[0] = 0; m.dst_q1[0] = 3; m.dst_q0[1] = 3; m.dst_q1[1] = 4; m.dst_pad[1] = 1; m.dst_q0[2] = 4; m.dst_q1[2] = 10;
        m.residual = p16; m.act = CRFP_ACT_LRELU01;
        fab(m, 0);
        crfp_probe_conv om = q;
        om.cout = 216; om.cout_split = 144; om.store = CRFP_PROBE_ST_OFFMASK; om.n_off_quads = 36; om.dst_q1[0] = 54;
        fab(om, 1);
        crfp_probe_conv ps = q;
        ps.cout = 64; ps.store = CRFP_PROBE_ST_PS; ps.ps_r = 4;
        fab(ps, 2);
        fab(two, 3); fab(a0, 4); fab(q, 5);
        void* const wsp = dev + (100ull << 32);
        const crfp_probe_conv* singles[] = {&m, &om, &ps, &two, &q};
        for (const crfp_probe_conv* c : singles)
            for (const auto& g : {std::initializer_list<int>{1, 1, 1}, {3, 17, 33}, {2, 9, 130}}) {
                const int n = g.begin()[0], h = g.begin()[1], w = g.begin()[2];
                EXPECT(crfp_conv_probe(CRFP_PROBE_SINGLE, c, nullptr, n, h, w, st, k, wsp, crfp_conv_probe_workspace_bytes(CRFP_PROBE_SINGLE, c, nullptr, n, h, w), nullptr) == 0);
                EXPECT(crfp_conv_probe_bf16(CRFP_PROBE_SINGLE, c, nullptr, n, h, w, st, k, wsp, crfp_conv_probe_workspace_bytes_bf16(CRFP_PROBE_SINGLE, c, nullptr, n, h, w), nullptr) == 0);
            }
        EXPECT(crfp_conv_probe(CRFP_PROBE_DUAL, &two, &m, 2, 8, 65, st, k, wsp, crfp_conv_probe_workspace_bytes(CRFP_PROBE_DUAL, &two, &m, 2, 8, 65), nullptr) == 0);
        EXPECT(crfp_conv_probe(CRFP_PROBE_DUAL, &two, &two, 2, 8, 65, st, k, wsp, crfp_conv_probe_workspace_bytes(CRFP_PROBE_DUAL, &two, &two, 2, 8, 65), nullptr) == 0);
        EXPECT(k[0] == CRFP_CONVK_SPLIT_DUAL);
        EXPECT(crfp_conv_probe_bf16(CRFP_PROBE_PAIR, &a0, &q, 2, 8, 62, st, k, wsp, crfp_conv_probe_workspace_bytes_bf16(CRFP_PROBE_PAIR, &a0, &q, 2, 8, 62), nullptr) == 0);
        EXPECT(crfp_conv_probe_bf16(CRFP_PROBE_PAIR, &a0, &two, 2, 8, 62, st, k, wsp, (size_t)1 << 40, nullptr) == CRFP_E_UNSUPPORTED);   // conv b must be 32 -> 32
        // the fp32 pair path: a whole call, the 32 -> 32 rule for conv b, and no pair under strict fp32
        EXPECT(crfp_conv_probe(CRFP_PROBE_PAIR_F32, &a0, &q, 2, 19, 130, st, k, wsp, crfp_conv_probe_workspace_bytes(CRFP_PROBE_PAIR_F32, &a0, &q, 2, 19, 130), nullptr) == 0);
        EXPECT(k[0] == CRFP_CONVK_SPLIT_PAIR && k[1] == CRFP_CONVK_SPLIT_PAIR);
        EXPECT(crfp_conv_probe(CRFP_PROBE_PAIR_F32, &a0, &two, 2, 8, 62, st, k, wsp, (size_t)1 << 40, nullptr) == CRFP_E_UNSUPPORTED);
        {
            crfp_probe_conv as = a0;
            as.strict = 1;
            EXPECT(crfp_conv_probe(CRFP_PROBE_PAIR_F32, &as, &q, 2, 8, 62, st, k, wsp, (size_t)1 << 40, nullptr) == CRFP_E_UNSUPPORTED);
        }
        EXPECT(crfp_conv_probe(CRFP_PROBE_S3_CHAIN, &a0, &two, 2, 8, 62, st, k, wsp, crfp_conv_probe_workspace_bytes(CRFP_PROBE_S3_CHAIN, &a0, &two, 2, 8, 62), nullptr) == 0);
        EXPECT(crfp_stub_launches() > l0);
    }
    // the narrow probe (test hook): the launchers' sizing functions (tiles and workgroups of launch_narrow's two branches, of the pair and of the
    // chain launcher), the kernel family per build, every refusal of the probe before the first launch, and the launchers' own refusals passed
    // through from whole calls on the stub
    {
        crfp_narrow_stencil q;
        std::memset(&q, 0, sizeof(q));
        q.nsrc = 1; q.src_kind[0] = CRFP_PROBE_SRC_Q4; q.src_nch[0] = 4; q.cout = 4; q.post_scale = 1.0f; q.gate_h = -1;
        crfp_narrow_stencil fed = q;      // the second / third stencil of a pair / chain: its quad is the stencil before it
        fed.nsrc = 0;
        crfp_narrow_stencil q2 = q, q3 = q;
        q2.nsrc = 2; q2.src_kind[1] = CRFP_PROBE_SRC_Q4; q2.src_nch[1] = 4;
        q3 = q2; q3.nsrc = 3; q3.src_kind[2] = CRFP_PROBE_SRC_FLOW2; q3.src_nch[2] = 2;
        crfp_narrow_report r;
        const long l0 = crfp_stub_launches();
        auto plan = [&](bool bf16, int mode, const crfp_narrow_stencil* a, const crfp_narrow_stencil* b, const crfp_narrow_stencil* c, int res, int h, int w) {
            std::memset(&r, 0xEE, sizeof(r));
            return bf16 ? crfp_narrow_probe_plan_bf16(mode, a, b, c, res, 1, h, w, &r) : crfp_narrow_probe_plan(mode, a, b, c, res, 1, h, w, &r);
        };
        // one tile; 17 x 65 = 2 x 2 tiles; a 650 x 2040 map = 41 x 32 = 1 312 tiles of 64 x 16, 41 x 34 = 1 394 of 60 x 16
        EXPECT(plan(false, CRFP_NPROBE_SINGLE, &q, nullptr, nullptr, 0, 1, 1) == 0 && r.kernel == CRFP_NARROWK_SEQ && r.kq == 1 && r.tiles == 1 && r.workgroups == 1);
        EXPECT(plan(true, CRFP_NPROBE_SINGLE, &q, nullptr, nullptr, 0, 17, 65) == 0 && r.kernel == CRFP_NARROWK_NARROW && r.epi == CRFP_NEPI_PLAIN && !r.gate && !r.st2 && r.tiles == 4 && r.workgroups == 4);
        // fp32 build: the quad-sequential form at four workgroups per CU whatever kq (1 024 slots -> shares of 2 -> 656 workgroups)
        EXPECT(plan(false, CRFP_NPROBE_SINGLE, &q3, nullptr, nullptr, 0, 650, 2040) == 0 && r.kernel == CRFP_NARROWK_SEQ && r.kq == 3 && r.tiles == 1312 && r.workgroups == 656);
        EXPECT(plan(false, CRFP_NPROBE_SINGLE, &q, nullptr, nullptr, 0, 512, 2048) == 0 && r.tiles == 1024 && r.workgroups == 1024);
        EXPECT(plan(false, CRFP_NPROBE_SINGLE, &q, nullptr, nullptr, 0, 513, 2048) == 0 && r.tiles == 1056 && r.workgroups == 528);
        // bf16 build: conv3x3_narrow_kernel at 5 / 3 / 2 workgroups per CU
        EXPECT(plan(true, CRFP_NPROBE_SINGLE, &q, nullptr, nullptr, 0, 650, 2040) == 0 && r.kernel == CRFP_NARROWK_NARROW && r.workgroups == 656);    // 1 280 slots: shares of 2
        EXPECT(plan(true, CRFP_NPROBE_SINGLE, &q2, nullptr, nullptr, 0, 650, 2040) == 0 && r.kq == 2 && r.workgroups == 656);                           // 768 slots: shares of 2
        EXPECT(plan(true, CRFP_NPROBE_SINGLE, &q3, nullptr, nullptr, 0, 650, 2040) == 0 && r.kq == 3 && r.workgroups == 438);                           // 512 slots: shares of 3
        {   // the forms that stay on conv3x3_narrow_kernel in the fp32 build: an epilogue, a gate, a second destination
            crfp_narrow_stencil e = q2;
            e.epi = CRFP_NEPI_BLEND;
            EXPECT(plan(false, CRFP_NPROBE_SINGLE, &e, nullptr, nullptr, 0, 650, 2040) == 0 && r.kernel == CRFP_NARROWK_NARROW && r.epi == CRFP_NEPI_BLEND && r.workgroups == 656);
            e.gate_h = 2;
            EXPECT(plan(false, CRFP_NPROBE_SINGLE, &e, nullptr, nullptr, 0, 72, 328) == 0 && r.kernel == CRFP_NARROWK_NARROW && r.gate && r.tiles == 30);
            e = q; e.dst2_on = 1;
            EXPECT(plan(false, CRFP_NPROBE_SINGLE, &e, nullptr, nullptr, 0, 17, 65) == 0 && r.kernel == CRFP_NARROWK_NARROW && r.st2 && !r.gate);
            e = q; e.epi = CRFP_NEPI_LAST; e.cout = 3;
            EXPECT(plan(false, CRFP_NPROBE_SINGLE, &e, nullptr, nullptr, 0, 16, 64) == 0 && r.kernel == CRFP_NARROWK_NARROW && r.epi == CRFP_NEPI_LAST);
            EXPECT(plan(false, CRFP_NPROBE_SINGLE, &e, nullptr, nullptr, 0, 17, 64) == CRFP_E_BADARG);                  // the x8 base needs multiples of 8
        }
        // pair: three workgroups per CU for one input quad, two otherwise; chain: 60-column tiles, three per CU
        EXPECT(plan(false, CRFP_NPROBE_PAIR, &q, &fed, nullptr, 0, 650, 2040) == 0 && r.kernel == CRFP_NARROWK_PAIR && r.kq == 1 && r.tiles == 1312 && r.workgroups == 656);
        EXPECT(plan(true, CRFP_NPROBE_PAIR, &q3, &fed, nullptr, 0, 650, 2040) == 0 && r.kq == 3 && r.workgroups == 438);
        EXPECT(plan(false, CRFP_NPROBE_CHAIN, &q2, &fed, &fed, 1, 650, 2040) == 0 && r.kernel == CRFP_NARROWK_CHAIN && r.kq == 2 && r.kqg == 0 && r.res && r.tiles == 1394 && r.workgroups == 697);
        EXPECT(plan(true, CRFP_NPROBE_CHAIN, &q, &fed, &q, 0, 16, 60) == 0 && r.kqg == 1 && !r.res && r.tiles == 1 && r.workgroups == 1);
        EXPECT(crfp_narrow_probe_plan(CRFP_NPROBE_SINGLE, &q, nullptr, nullptr, 0, 1, 16, 64, nullptr) == CRFP_E_BADARG);
        // the probe's own refusals, sizes-only and both builds
        auto refused = [&](int mode, const crfp_narrow_stencil* a, const crfp_narrow_stencil* b, const crfp_narrow_stencil* c, const char* text) {
            const bool zero = crfp_narrow_probe_workspace_bytes(mode, a, b, c, 0, 2, 16, 64) == 0 && std::strstr(crfp_last_error_string(), text) != nullptr;
            return zero && crfp_narrow_probe_workspace_bytes_bf16(mode, a, b, c, 0, 2, 16, 64) == 0 && std::strstr(crfp_last_error_string(), text) != nullptr;
        };
        EXPECT(crfp_narrow_probe_workspace_bytes(CRFP_NPROBE_SINGLE, &q, nullptr, nullptr, 0, 2, 16, 64) > 2ull * 2 * 16 * 64 * 16);
        EXPECT(crfp_narrow_probe_workspace_bytes_bf16(CRFP_NPROBE_SINGLE, &q, nullptr, nullptr, 0, 2, 16, 64) < crfp_narrow_probe_workspace_bytes(CRFP_NPROBE_SINGLE, &q, nullptr, nullptr, 0, 2, 16, 64));
        EXPECT(refused(3, &q, &fed, &fed, "unknown mode") && refused(-1, &q, nullptr, nullptr, "unknown mode"));
        EXPECT(refused(CRFP_NPROBE_PAIR, &q, nullptr, nullptr, "null stencil") && refused(CRFP_NPROBE_CHAIN, &q, &fed, nullptr, "null stencil"));
        EXPECT(refused(CRFP_NPROBE_PAIR, &q, &q, nullptr, "a pair's second stencil reads one quad"));
        EXPECT(refused(CRFP_NPROBE_CHAIN, &q, &q, &fed, "at most 0 global quad") && refused(CRFP_NPROBE_CHAIN, &q, &fed, &q2, "at most 1 global quad"));
        for (int bad = 0; bad < 12; ++bad) {
            crfp_narrow_stencil d = q;
            switch (bad) {
                case 0: d.cout = 5; break;
                case 1: d.cout = 0; break;
                case 2: d.nsrc = 4; break;                                     // more than 3 input quads
                case 3: d.nsrc = 0; break;
                case 4: d.src_kind[0] = CRFP_PROBE_SRC_UNSHUF4; break;
                case 5: d.src_nch[0] = 5; break;                               // a source is one quad
                case 6: d.act = CRFP_ACT_TANH; break;                          // no engine item uses tanh / sigmoid
                case 7: d.epi = 4; break;
                case 8: d.cout_split = 4; break;
                case 9: d.src_kind[0] = CRFP_PROBE_SRC_FLOW2; d.src_nch[0] = 2; d.src_pad = 1; break;   // only a Q4 source is padded
                case 10: d.gate_h = 4; break;
                default: d.epi = CRFP_NEPI_OFFMASK3; d.dst_pad = 1; break;     // only Q4 destinations are padded
            }
            EXPECT(crfp_narrow_probe_workspace_bytes(CRFP_NPROBE_SINGLE, &d, nullptr, nullptr, 0, 2, 16, 64) == 0);
            EXPECT(crfp_narrow_probe_workspace_bytes_bf16(CRFP_NPROBE_SINGLE, &d, nullptr, nullptr, 0, 2, 16, 64) == 0);
        }
        {
            crfp_narrow_stencil g = q;
            g.gate_h = 1;
            EXPECT(crfp_narrow_probe_workspace_bytes(CRFP_NPROBE_SINGLE, &g, nullptr, nullptr, 0, 2, 16, 66) == 0);   // the mask is read four bytes at a time
            crfp_narrow_stencil gf = fed;
            gf.gate_h = 0;
            EXPECT(refused(CRFP_NPROBE_PAIR, &q, &gf, nullptr, "no mask-gated form of a pair or chain"));
            g.dst2_on = 1;
            EXPECT(refused(CRFP_NPROBE_SINGLE, &g, nullptr, nullptr, "no mask-gated form with a second destination"));
            crfp_narrow_stencil a2 = q;
            a2.dst2_on = 1;
            EXPECT(refused(CRFP_NPROBE_PAIR, &a2, &fed, nullptr, "only the last stencil"));
            crfp_narrow_stencil pd = q;
            pd.src_pad = 1;
            EXPECT(refused(CRFP_NPROBE_PAIR, &pd, &fed, nullptr, "unpadded tensors"));
        }
        // the call: null tensors, null status / report, a short workspace -- all before the first launch
        unsigned* const st = reinterpret_cast<unsigned*>(16);
        const size_t w32 = crfp_narrow_probe_workspace_bytes(CRFP_NPROBE_SINGLE, &q, nullptr, nullptr, 0, 2, 16, 64);
        EXPECT(crfp_narrow_probe(CRFP_NPROBE_SINGLE, &q, nullptr, nullptr, 0, 2, 16, 64, nullptr, st, &r, p16, w32, nullptr) == CRFP_E_BADARG);   // null tensors
        EXPECT(crfp_stub_launches() == l0);
        char* const dev = reinterpret_cast<char*>(0x300000000000ull);
        auto fab = [&](crfp_narrow_stencil& d, int slot) {
            float* const base = reinterpret_cast<float*>(dev + ((size_t)slot << 32));
            for (int i = 0; i < 3; ++i) d.src[i] = base + (i << 24);
            d.weight = base + (5 << 24); d.bias = base + (6 << 24); d.weight2 = base + (7 << 24); d.bias2 = base + (8 << 24);
            d.flow = base + (9 << 24); d.base_lr = base + (10 << 24); d.mask = reinterpret_cast<const unsigned char*>(base + (11 << 24));
            d.dst = base + (12 << 24); d.dst_raw = base + (13 << 24); d.dst2 = base + (14 << 24); d.dst2_raw = base + (15 << 24);
        };
        fab(q, 0); fab(fed, 1); fab(q2, 2); fab(q3, 3);
        void* const wsp = dev + (100ull << 32);
        EXPECT(crfp_narrow_probe(CRFP_NPROBE_SINGLE, &q, nullptr, nullptr, 0, 2, 16, 64, nullptr, nullptr, &r, wsp, w32, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_narrow_probe(CRFP_NPROBE_SINGLE, &q, nullptr, nullptr, 0, 2, 16, 64, nullptr, st, nullptr, wsp, w32, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_narrow_probe(CRFP_NPROBE_SINGLE, &q, nullptr, nullptr, 0, 2, 16, 64, nullptr, st, &r, wsp, w32 - 1, nullptr) == CRFP_E_WORKSPACE);
        EXPECT(crfp_narrow_probe(CRFP_NPROBE_SINGLE, &q, nullptr, nullptr, 0, 2, 16, 64, nullptr, st, &r, nullptr, w32, nullptr) == CRFP_E_WORKSPACE);
        EXPECT(crfp_stub_launches() == l0);
        // accepted calls on the stub runtime, device pointers fabricated: every mode, epilogue and pad, both builds
        auto call = [&](bool bf16, int mode, const crfp_narrow_stencil* a, const crfp_narrow_stencil* b, const crfp_narrow_stencil* c, int res, int n, int h, int w) {
            const size_t bytes = bf16 ? crfp_narrow_probe_workspace_bytes_bf16(mode, a, b, c, res, n, h, w) : crfp_narrow_probe_workspace_bytes(mode, a, b, c, res, n, h, w);
            if (!bytes) return -1000;
            return bf16 ? crfp_narrow_probe_bf16(mode, a, b, c, res, n, h, w, st, st, &r, wsp, bytes, nullptr)
                        : crfp_narrow_probe(mode, a, b, c, res, n, h, w, st, st, &r, wsp, bytes, nullptr);
        };
        crfp_narrow_stencil win = q, blend = q2, lastq = q, om = q, st2 = q, gated = q2;
        win.src_pad = 37; win.dst_pad = 37; win.residual = p16; win.act = CRFP_ACT_LRELU01;
        blend.epi = CRFP_NEPI_BLEND;
        lastq.epi = CRFP_NEPI_LAST; lastq.cout = 1; lastq.y_only = 1;
        om.epi = CRFP_NEPI_OFFMASK3; om.cout = 3; om.cout_split = 2;
        st2.dst2_on = 1; st2.src_pad = 1; st2.dst_pad = 1;
        gated.gate_h = 3;
        const crfp_narrow_stencil* singles[] = {&q, &q2, &q3, &win, &blend, &lastq, &om, &st2, &gated};
        for (const crfp_narrow_stencil* c : singles)
            for (const auto& g : {std::initializer_list<int>{1, 8, 8}, {3, 16, 64}, {2, 72, 328}})
                for (int bf16 = 0; bf16 < 2; ++bf16)
                    EXPECT(call(bf16 != 0, CRFP_NPROBE_SINGLE, c, nullptr, nullptr, 0, g.begin()[0], g.begin()[1], g.begin()[2]) == 0);
        crfp_narrow_stencil fed_om = fed, fed_st2 = fed;
        fed_om.epi = CRFP_NEPI_OFFMASK3; fed_om.cout = 3; fed_om.cout_split = 2;
        fed_st2.dst2_on = 1; fed_st2.residual = p16;
        for (int bf16 = 0; bf16 < 2; ++bf16) {
            EXPECT(call(bf16 != 0, CRFP_NPROBE_PAIR, &q3, &fed_om, nullptr, 0, 2, 17, 65) == 0 && r.kernel == CRFP_NARROWK_PAIR && r.epi == CRFP_NEPI_OFFMASK3);
            EXPECT(call(bf16 != 0, CRFP_NPROBE_PAIR, &q, &fed_st2, nullptr, 0, 2, 17, 65) == 0);
            EXPECT(call(bf16 != 0, CRFP_NPROBE_CHAIN, &q2, &fed, &fed_st2, 1, 2, 17, 61) == CRFP_E_UNSUPPORTED);      // c has a residual of its own
            EXPECT(call(bf16 != 0, CRFP_NPROBE_CHAIN, &q3, &fed, &q, 0, 2, 17, 61) == 0 && r.kernel == CRFP_NARROWK_CHAIN && r.kqg == 1);
            EXPECT(call(bf16 != 0, CRFP_NPROBE_CHAIN, &q, &fed, &q, 1, 2, 17, 61) == CRFP_E_UNSUPPORTED);             // a residual chain has no global quad in c
            EXPECT(std::strstr(crfp_last_error_string(), "conv_narrow_chain narrow_probe:chain: unsupported chain (kqA=1 kqB=1 kqC=2 res=1)") != nullptr);
        }
        // the launchers' own refusals come back unchanged: chain shapes per build, the gated and the second-destination forms, a residual on a pair's a
        EXPECT(call(false, CRFP_NPROBE_CHAIN, &q3, &fed, &fed, 1, 2, 17, 61) == 0 && call(true, CRFP_NPROBE_CHAIN, &q3, &fed, &fed, 1, 2, 17, 61) == CRFP_E_UNSUPPORTED);
        EXPECT(call(false, CRFP_NPROBE_CHAIN, &q, &fed, &fed, 0, 2, 17, 61) == 0 && call(true, CRFP_NPROBE_CHAIN, &q, &fed, &fed, 0, 2, 17, 61) == CRFP_E_UNSUPPORTED);
        {
            crfp_narrow_stencil g3 = q3, gb = q, d2 = q2, ra = q;
            g3.gate_h = 0; gb.gate_h = 0; gb.epi = CRFP_NEPI_BLEND; d2.dst2_on = 1; ra.residual = p16;
            for (int bf16 = 0; bf16 < 2; ++bf16) {
                EXPECT(call(bf16 != 0, CRFP_NPROBE_SINGLE, &g3, nullptr, nullptr, 0, 2, 16, 64) == CRFP_E_UNSUPPORTED);
                EXPECT(std::strstr(crfp_last_error_string(), "conv_narrow narrow_probe:a: no mask-gated form for kq=3 epi=0") != nullptr);
                EXPECT(call(bf16 != 0, CRFP_NPROBE_SINGLE, &gb, nullptr, nullptr, 0, 2, 16, 64) == CRFP_E_UNSUPPORTED);
                EXPECT(call(bf16 != 0, CRFP_NPROBE_SINGLE, &d2, nullptr, nullptr, 0, 2, 16, 64) == CRFP_E_UNSUPPORTED);
                EXPECT(std::strstr(crfp_last_error_string(), "a second destination needs a plain one-quad stencil (kq=2 epi=0)") != nullptr);
                EXPECT(call(bf16 != 0, CRFP_NPROBE_PAIR, &ra, &fed, nullptr, 0, 2, 16, 64) == CRFP_E_UNSUPPORTED);
                EXPECT(std::strstr(crfp_last_error_string(), "conv_narrow_pair narrow_probe:pair: unsupported pair") != nullptr);
            }
        }
        EXPECT(crfp_stub_launches() > l0);
    }
    // ---- whole engine calls on the stub runtime (tools/asan_host/hip_stub.cpp: every HIP call succeeds, no kernel runs): the host side of a
    // call -- argument checks, Layout arenas, the launch-argument tables of ~50 launches per frame, the fork / join of the side stream, the
    // per-thread stream table and crfp_shutdown() -- under the sanitizers.  Device pointers are fabricated and never dereferenced on the host.
    {
        char* const dev = reinterpret_cast<char*>(0x100000000000ull);
        float* const lrs = reinterpret_cast<float*>(dev), *const fvs = reinterpret_cast<float*>(dev + (1ull << 36));
        const uint8_t* const mks = reinterpret_cast<const uint8_t*>(dev + (2ull << 36));
        float* const out = reinterpret_cast<float*>(dev + (3ull << 36));
        void* const wsp = dev + (4ull << 36);
        void* const pk = dev + (5ull << 36);
        void* const stream = nullptr;
        const float* params[256];
        for (int i = 0; i < 256; ++i) params[i] = reinterpret_cast<const float*>(dev + (6ull << 36) + ((size_t)i << 24));
        const long l0 = crfp_stub_launches();
        EXPECT(crfp_dsv_pack_weights(params, 0, pk, crfp_dsv_packed_weight_bytes(0), stream) == 0);
        EXPECT(crfp_dsv_pack_weights_bf16(params, 0, pk, crfp_dsv_packed_weight_bytes_bf16(0), stream) == 0);
        EXPECT(crfp_cra_pack_weights(params, 0, pk, crfp_cra_packed_weight_bytes(0), stream) == 0);
        EXPECT(crfp_simple_pack_weights(params, 1, pk, crfp_simple_packed_weight_bytes(1), stream) == 0);
        EXPECT(crfp_dense_pack_weights_bf16(params, 0, pk, crfp_dense_packed_weight_bytes_bf16(0), stream) == 0);
        EXPECT(crfp_dense_pack_weights(params, 0, pk, crfp_dsv_packed_weight_bytes(0), stream) != 0);   // the wider main.0 images need more
        EXPECT(crfp_rt_pack_weights(params, 0, pk, crfp_rt_packed_weight_bytes(0), stream) == 0);
        EXPECT(crfp_dsv_pack_weights(params, 0, pk, 1024, stream) != 0);   // packed buffer too small
        const int geo[][2] = {{20, 36}, {33, 47}, {101, 170}, {180, 320}};
        for (const auto& g : geo) {
            const int h = g[0], w = g[1];
            for (int t : {1, 3, 9}) {
                EXPECT(crfp_dsv_forward_clip(pk, 0, lrs, fvs, mks, out, t, h, w, wsp, crfp_dsv_workspace_bytes(t, h, w), stream) == 0);
                EXPECT(crfp_dsv_forward_clip(pk, CRFP_DSV_SINGLE_STREAM | CRFP_DSV_Y_ONLY, lrs, fvs, mks, out, t, h, w, wsp, crfp_dsv_workspace_bytes(t, h, w), stream) == 0);
                EXPECT(crfp_dsv_forward_clip(pk, CRFP_DSV_STRICT_F32, lrs, fvs, mks, out, t, h, w, wsp, crfp_dsv_workspace_bytes(t, h, w), stream) == 0);
                EXPECT(crfp_dsv_forward_clip_bf16(pk, 0, lrs, fvs, mks, out, t, h, w, wsp, crfp_dsv_workspace_bytes_bf16(t, h, w), stream) == 0);
                for (int n : {2, 4}) {
                    EXPECT(crfp_dsv_forward_batch(pk, 0, lrs, fvs, mks, out, n, t, h, w, wsp, crfp_dsv_batch_workspace_bytes(n, t, h, w), stream) == 0);
                    EXPECT(crfp_dsv_forward_batch_bf16(pk, 0, lrs, fvs, mks, out, n, t, h, w, wsp, crfp_dsv_batch_workspace_bytes_bf16(n, t, h, w), stream) == 0);
                    EXPECT(crfp_cra_forward_batch(pk, 0, lrs, fvs, mks, out, n, t, h, w, wsp, crfp_cra_batch_workspace_bytes(n, t, h, w), stream) == 0);
                    EXPECT(crfp_simple_forward_batch(pk, n == 2 ? CRFP_DSV_STRICT_F32 : 0, lrs, fvs, mks, out, n, t, h, w, wsp, crfp_simple_batch_workspace_bytes(n, t, h, w), stream) == 0);
                    EXPECT(crfp_dense_forward_batch(pk, CRFP_DSV_SINGLE_STREAM, lrs, fvs, mks, out, n, t, h, w, wsp, crfp_dense_batch_workspace_bytes(n, t, h, w), stream) == 0);
                    EXPECT(crfp_dense_forward_batch_bf16(pk, 0, lrs, fvs, mks, out, n, t, h, w, wsp, crfp_dense_batch_workspace_bytes_bf16(n, t, h, w), stream) == 0);
                    EXPECT(crfp_simple_forward_batch(pk, 0, lrs, fvs, mks, out, n, t, h, w, wsp, crfp_dsv_batch_workspace_bytes(n, t, h, w), stream) != 0);   // CRFP_DSV's smaller workspace
                    EXPECT(crfp_dsv_forward_batch(pk, 0, lrs, fvs, mks, out, n, t, h, w, wsp, crfp_dsv_batch_workspace_bytes(n, t, h, w) - 1, stream) != 0);
                }
            }
            // pre-work groups (engine.hip, prework_group): (n, t) around every rule boundary -- two frames, one full group, a tail group, a third
            // group on the first one's slots, a chunked 40-frame clip; whole clips of a small batch, a batch just past the item cap, a chunked batch
            const int grouped[][2] = {{1, 2}, {1, 8}, {1, 16}, {1, 17}, {1, 40}, {2, 3}, {2, 4}, {2, 5}, {2, 17}};
            for (const auto& c : grouped) {
                const int n = c[0], t = c[1];
                EXPECT(crfp_dsv_forward_batch(pk, 0, lrs, fvs, mks, out, n, t, h, w, wsp, crfp_dsv_batch_workspace_bytes(n, t, h, w), stream) == 0);
                EXPECT(crfp_dsv_forward_batch(pk, CRFP_DSV_SINGLE_STREAM, lrs, fvs, mks, out, n, t, h, w, wsp, crfp_dsv_batch_workspace_bytes(n, t, h, w), stream) == 0);
                EXPECT(crfp_dsv_forward_batch_bf16(pk, 0, lrs, fvs, mks, out, n, t, h, w, wsp, crfp_dsv_batch_workspace_bytes_bf16(n, t, h, w), stream) == 0);
                EXPECT(crfp_cra_forward_batch(pk, 0, lrs, fvs, mks, out, n, t, h, w, wsp, crfp_cra_batch_workspace_bytes(n, t, h, w), stream) == 0);
                EXPECT(crfp_cra_forward_batch(pk, CRFP_DSV_SINGLE_STREAM, lrs, fvs, mks, out, n, t, h, w, wsp, crfp_cra_batch_workspace_bytes(n, t, h, w), stream) == 0);
                EXPECT(crfp_dense_forward_batch_bf16(pk, 0, lrs, fvs, mks, out, n, t, h, w, wsp, crfp_dense_batch_workspace_bytes_bf16(n, t, h, w), stream) == 0);
                EXPECT(crfp_dsv_forward_batch(pk, 0, lrs, fvs, mks, out, n, t, h, w, wsp, crfp_dsv_batch_workspace_bytes(n, t, h, w) - 1, stream) != 0);
            }
            // one frame per call: first call, then steady calls with and without the resident-inputs promise, with a regional mask, in a batch
            const size_t sws = crfp_dsv_batch_workspace_bytes(1, 1, h, w);
            EXPECT(crfp_dsv_stream_frame(pk, 0, lrs, nullptr, fvs, mks, nullptr, out, 1, h, w, wsp, sws, stream) == 0);
            EXPECT(crfp_dsv_stream_frame(pk, 0, lrs, lrs, fvs, mks, nullptr, out, 0, h, w, wsp, sws, stream) == 0);
            EXPECT(crfp_dsv_stream_frame(pk, 0, lrs, lrs, fvs, mks, mks, out, 0, h, w, wsp, sws, stream) == 0);
            EXPECT(crfp_dsv_stream_frame(pk, CRFP_DSV_INPUTS_RESIDENT, lrs, nullptr, fvs, mks, nullptr, out, 1, h, w, wsp, sws, stream) == 0);
            for (int k = 0; k < 3; ++k)
                EXPECT(crfp_dsv_stream_frame(pk, CRFP_DSV_INPUTS_RESIDENT, lrs, nullptr, fvs, mks, nullptr, out, 0, h, w, wsp, sws, stream) == 0);
            EXPECT(crfp_dsv_stream_frame_bf16(pk, 0, lrs, lrs, fvs, mks, nullptr, out, 0, h, w, wsp, crfp_dsv_batch_workspace_bytes_bf16(1, 1, h, w), stream) == 0);
            EXPECT(crfp_dsv_stream_batch(pk, 0, lrs, lrs, fvs, mks, nullptr, out, 0, 3, h, w, wsp, crfp_dsv_batch_workspace_bytes(3, 1, h, w), stream) == 0);
            EXPECT(crfp_dsv_stream_batch(pk, 0, lrs, lrs, fvs, mks, mks, out, 0, 3, h, w, wsp, crfp_dsv_batch_workspace_bytes(3, 1, h, w), stream) != 0);   // fg needs n = 1
            EXPECT(crfp_dsv_stream_batch(pk, 0, lrs, lrs, fvs, mks, nullptr, out, 0, 33, h, w, wsp, (size_t)1 << 44, stream) != 0);                          // n <= 32
            // the streaming forms of the CRFP_simple / CRFP / CRFP_DSV_CRA wirings (MRCF_simple_v13 / v15 / v18_cra): the same calls on their own workspaces
            decltype(&crfp_simple_stream_batch) abl[] = {crfp_simple_stream_batch, crfp_dense_stream_batch, crfp_cra_stream_batch,
                                                         crfp_simple_stream_batch_bf16, crfp_dense_stream_batch_bf16, crfp_cra_stream_batch_bf16};
            decltype(&crfp_simple_batch_workspace_bytes) abl_ws[] = {crfp_simple_batch_workspace_bytes, crfp_dense_batch_workspace_bytes, crfp_cra_batch_workspace_bytes,
                                                                      crfp_simple_batch_workspace_bytes_bf16, crfp_dense_batch_workspace_bytes_bf16,
                                                                      crfp_cra_batch_workspace_bytes_bf16};
            for (int k = 0; k < 6; ++k) {
                const auto sb = abl[k];
                const size_t w1 = abl_ws[k](1, 1, h, w), w3 = abl_ws[k](3, 1, h, w);
                EXPECT(sb(pk, 0, lrs, nullptr, fvs, mks, nullptr, out, 1, 1, h, w, wsp, w1, stream) == 0);                                // first frame
                EXPECT(sb(pk, k < 3 ? CRFP_DSV_STRICT_F32 : 0, lrs, lrs, fvs, mks, nullptr, out, 0, 1, h, w, wsp, w1, stream) == 0);       // next frame
                EXPECT(sb(pk, CRFP_DSV_SINGLE_STREAM, lrs, lrs, fvs, mks, mks, out, 0, 1, h, w, wsp, w1, stream) == 0);                   // fg: ignored
                EXPECT(sb(pk, CRFP_DSV_INPUTS_RESIDENT, lrs, nullptr, fvs, mks, nullptr, out, 1, 1, h, w, wsp, w1, stream) == 0);         // resident
                for (int j = 0; j < 3; ++j)
                    EXPECT(sb(pk, CRFP_DSV_INPUTS_RESIDENT | CRFP_DSV_Y_ONLY, lrs, nullptr, fvs, mks, nullptr, out, 0, 1, h, w, wsp, w1, stream) == 0);
                EXPECT(sb(pk, 0, lrs, nullptr, fvs, mks, nullptr, out, 1, 3, h, w, wsp, w3, stream) == 0);                                // n = 3
                EXPECT(sb(pk, 0, lrs, lrs, fvs, mks, mks, out, 0, 3, h, w, wsp, w3, stream) == 0);                                        // fg with n > 1: accepted
                EXPECT(sb(pk, CRFP_DSV_INPUTS_RESIDENT, lrs, nullptr, fvs, mks, mks, out, 1, 3, h, w, wsp, w3, stream) == 0);
                EXPECT(sb(pk, CRFP_DSV_INPUTS_RESIDENT, lrs, nullptr, fvs, mks, nullptr, out, 0, 3, h, w, wsp, w3, stream) == 0);
                EXPECT(sb(pk, 0, lrs, lrs, fvs, mks, nullptr, out, 0, 33, h, w, wsp, (size_t)1 << 44, stream) == CRFP_E_UNSUPPORTED);    // n <= 32
                const size_t dsv_ws = k < 3 ? crfp_dsv_batch_workspace_bytes(1, 1, h, w) : crfp_dsv_batch_workspace_bytes_bf16(1, 1, h, w);
                EXPECT(dsv_ws < w1 && sb(pk, 0, lrs, lrs, fvs, mks, nullptr, out, 0, 1, h, w, wsp, dsv_ws, stream) == CRFP_E_WORKSPACE);   // CRFP_DSV-sized
                void* const fresh = dev + (7ull << 36) + ((size_t)(k * 8 + (h & 7)) << 30);   // a workspace no sequence started on
                EXPECT(sb(pk, CRFP_DSV_INPUTS_RESIDENT, lrs, nullptr, fvs, mks, nullptr, out, 0, 1, h, w, fresh, w1, stream) == CRFP_E_BADARG);   // resident, no first call
                EXPECT(sb(pk, 0, lrs, nullptr, fvs, mks, nullptr, out, 0, 1, h, w, wsp, w1, stream) == CRFP_E_BADARG);                   // no previous frame
                if (k >= 3) EXPECT(sb(pk, CRFP_DSV_STRICT_F32, lrs, lrs, fvs, mks, nullptr, out, 0, 1, h, w, wsp, w1, stream) == CRFP_E_UNSUPPORTED);
            }
        }
        EXPECT(crfp_rt_forward_clip(pk, 0, lrs, fvs, out, 5, 135, 240, 96, 96, 720, 720, wsp, crfp_rt_workspace_bytes(5, 135, 240, 96, 96, 720, 720), stream) == 0);
        EXPECT(crfp_rt_forward_clip(pk, CRFP_DSV_STRICT_F32, lrs, fvs, out, 5, 135, 240, 96, 96, 720, 720, wsp, (size_t)1 << 40, stream) != 0);
        // the regional debug fetch: every refusal before the first launch, the size query launches nothing, a fetch is one launch or one copy
        {
            int c = -1, hh = -1, ww = -1;
            const long l1 = crfp_stub_launches();
            EXPECT(crfp_rt_debug_fetch(nullptr, 5, 135, 240, 96, 96, 720, 720, wsp, out, &c, &hh, &ww, stream) == CRFP_E_BADARG);
            EXPECT(std::strstr(crfp_last_error_string(), "null") != nullptr);
            EXPECT(crfp_rt_debug_fetch("state", 5, 135, 240, 96, 96, 720, 720, nullptr, out, &c, &hh, &ww, stream) == CRFP_E_BADARG);
            EXPECT(crfp_rt_debug_fetch("no_such_buffer", 5, 135, 240, 96, 96, 720, 720, wsp, out, &c, &hh, &ww, stream) == CRFP_E_BADARG);
            EXPECT(std::strstr(crfp_last_error_string(), "unknown buffer 'no_such_buffer'") != nullptr);
            EXPECT(crfp_rt_debug_fetch("", 5, 135, 240, 96, 96, 720, 720, wsp, out, nullptr, nullptr, nullptr, stream) == CRFP_E_BADARG);
            EXPECT(crfp_rt_debug_fetch("state", 5, 135, 240, 96, 96, 724, 720, wsp, out, &c, &hh, &ww, stream) == CRFP_E_BADARG);    // warp_size no multiple of 8
            EXPECT(std::strstr(crfp_last_error_string(), "warp_size") != nullptr);
            EXPECT(crfp_rt_debug_fetch("state", 0, 135, 240, 96, 96, 720, 720, wsp, out, &c, &hh, &ww, stream) == CRFP_E_BADARG);
            EXPECT(crfp_rt_debug_fetch("state", 5, 135, 240, 2000, 96, 720, 720, wsp, nullptr, &c, &hh, &ww, stream) == CRFP_E_BADARG);
            EXPECT(crfp_rt_debug_fetch("state_w", 1, 135, 240, 96, 96, 720, 720, wsp, nullptr, &c, &hh, &ww, stream) == CRFP_E_BADARG);  // one frame warps nothing
            EXPECT(std::strstr(crfp_last_error_string(), "frames >= 1") != nullptr);
            EXPECT(c == -1 && hh == -1 && ww == -1);                                                                                   // a refusal fills nothing in
            EXPECT(crfp_rt_debug_fetch("state", 1, 135, 240, 96, 96, 720, 720, wsp, nullptr, &c, &hh, &ww, stream) == 1 && c == 4 && hh == 720 && ww == 720);
            EXPECT(crfp_rt_debug_fetch("flow_lr", 5, 135, 240, 96, 96, 720, 720, wsp, nullptr, &c, &hh, &ww, stream) == 4 && c == 4 && hh == 90 && ww == 90);
            EXPECT(crfp_rt_debug_fetch("x_lr", 5, 135, 240, 96, 96, 720, 720, wsp, nullptr, &c, &hh, &ww, stream) == 5 && c == 32 && hh == 135 && ww == 240);
            EXPECT(crfp_rt_debug_fetch("x_hr", 5, 135, 240, 96, 80, 720, 720, wsp, nullptr, &c, &hh, &ww, stream) == 5 && c == 4 && hh == 96 && ww == 80);
            EXPECT(crfp_rt_debug_fetch("carry", 5, 135, 240, 96, 96, 720, 712, wsp, nullptr, &c, &hh, &ww, stream) == 1 && c == 24 && hh == 180 && ww == 178);
            EXPECT(crfp_rt_debug_fetch("offfeat1", 5, 135, 240, 96, 96, 720, 720, wsp, nullptr, &c, &hh, &ww, stream) == 1 && c == 32 && hh == 180 && ww == 180);
            EXPECT(crfp_rt_debug_fetch("flow8", 5, 135, 240, 96, 96, 720, 720, wsp, nullptr, &c, &hh, &ww, stream) == 1 && c == 2 && hh == 720 && ww == 720);
            EXPECT(crfp_rt_debug_fetch("feat2", 5, 135, 240, 96, 96, 720, 720, wsp, nullptr, nullptr, nullptr, nullptr, stream) == 1);
            EXPECT(crfp_rt_debug_fetch("feat2", 5, 135, 240, 96, 96, 720, 720, wsp, nullptr, &c, &hh, &ww, stream) == 1 && c == 4 && hh == 1080 && ww == 1920);
            EXPECT(crfp_stub_launches() == l1);
            const char* const names[] = {"flow_lr", "x_lr", "x_hr", "state", "state_w", "prev2", "prev2w", "carry", "carryw", "offfeat0", "offfeat1", "offfeat2",
                                         "aligned0", "aligned1", "aligned2", "poff", "al3", "feat2", "flow2", "flow8", "win", "upw"};
            for (const char* nm : names)
                for (int t : {2, 5})
                    EXPECT(crfp_rt_debug_fetch(nm, t, 135, 240, 96, 96, 720, 720, wsp, out, nullptr, nullptr, nullptr, stream) == 0);
            EXPECT(crfp_stub_launches() == l1 + 2 * (22 - 5));   // the two flow fields and the three split-fp16 images are copies
        }
        // the clip wirings' debug fetch: each reads its own Layout (cra.* exists for cra only, prop0 is 32 channels wide for simple / dense),
        // refusals and size queries launch nothing, frame-slot names answer with and without ".1"
        {
            typedef int (*fetch_fn)(const char*, int, int, int, const void*, float*, int*, int*, int*, void*);
            const fetch_fn fetch[8] = {crfp_dsv_debug_fetch, crfp_cra_debug_fetch, crfp_simple_debug_fetch, crfp_dense_debug_fetch,
                                       crfp_dsv_debug_fetch_bf16, crfp_cra_debug_fetch_bf16, crfp_simple_debug_fetch_bf16, crfp_dense_debug_fetch_bf16};
            const long l1 = crfp_stub_launches();
            for (int k = 0; k < 8; ++k) {
                const int wiring = k % 4;   // 0 dsv, 1 cra, 2 simple, 3 dense
                int c = -1, hh = -1, ww = -1;
                EXPECT(fetch[k](nullptr, 3, 33, 47, wsp, out, &c, &hh, &ww, stream) == CRFP_E_BADARG);
                EXPECT(fetch[k]("x_hr", 3, 33, 47, nullptr, out, &c, &hh, &ww, stream) == CRFP_E_BADARG);
                EXPECT(fetch[k]("x_hr", 0, 33, 47, wsp, nullptr, &c, &hh, &ww, stream) == CRFP_E_BADARG);
                EXPECT(fetch[k]("x_hr", 3, 7, 47, wsp, nullptr, &c, &hh, &ww, stream) == CRFP_E_BADARG);
                EXPECT(fetch[k]("no_such_buffer", 3, 33, 47, wsp, out, &c, &hh, &ww, stream) == CRFP_E_BADARG);
                EXPECT(std::strstr(crfp_last_error_string(), "unknown buffer 'no_such_buffer'") != nullptr);
                EXPECT(c == -1 && hh == -1 && ww == -1);
                EXPECT(fetch[k]("prop0", 3, 33, 47, wsp, nullptr, &c, &hh, &ww, stream) == 1 && c == (wiring >= 2 ? 32 : 24) && hh == 66 && ww == 94);
                EXPECT(fetch[k]("prop0.1", 2, 33, 47, wsp, nullptr, &c, &hh, &ww, stream) == 1 && c == (wiring >= 2 ? 32 : 24));
                EXPECT(fetch[k]("prop_a", 3, 33, 47, wsp, nullptr, &c, &hh, &ww, stream) == 1 && c == (wiring >= 2 ? 32 : 24));
                EXPECT(fetch[k]("state_hr", 3, 33, 47, wsp, nullptr, &c, &hh, &ww, stream) == 1 && c == 4 && hh == 264 && ww == 376);
                EXPECT(fetch[k]("flow_lr", 3, 33, 47, wsp, nullptr, &c, &hh, &ww, stream) == 2 && c == 4 && hh == 33 && ww == 47);
                for (const char* nm : {"cra.s1", "cra.a", "cra.b", "cra.lv0", "cra.lv1.1", "cra.lv2", "cra.y", "cra.fused"}) {
                    const int n = fetch[k](nm, 3, 33, 47, wsp, nullptr, &c, &hh, &ww, stream);
                    EXPECT(wiring == 1 ? n >= 1 : n == CRFP_E_BADARG);
                }
                if (wiring == 1) {
                    EXPECT(fetch[k]("cra.s1", 3, 33, 47, wsp, nullptr, &c, &hh, &ww, stream) == 3 && c == 4 && hh == 264 && ww == 376);   // a group's items
                    EXPECT(fetch[k]("cra.lv1", 3, 33, 47, wsp, nullptr, &c, &hh, &ww, stream) == 1 && c == 16 && hh == 66 && ww == 94);
                    EXPECT(fetch[k]("cra.fused", 3, 33, 47, wsp, nullptr, &c, &hh, &ww, stream) == 1 && c == 32 && hh == 66 && ww == 94);
                }
            }
            EXPECT(crfp_stub_launches() == l1);
            for (int k = 0; k < 8; ++k) {
                EXPECT(fetch[k]("prop_b", 3, 33, 47, wsp, out, nullptr, nullptr, nullptr, stream) == 0);
                EXPECT(fetch[k]("flow2.1", 3, 33, 47, wsp, out, nullptr, nullptr, nullptr, stream) == 0);   // a copy, not a launch
                if (k % 4 == 1) EXPECT(fetch[k]("cra.lv0.1", 3, 33, 47, wsp, out, nullptr, nullptr, nullptr, stream) == 0);
            }
            EXPECT(crfp_stub_launches() == l1 + 8 + 2);
        }
        EXPECT(crfp_fnet_forward(pk, lrs, lrs, out, 2, 180, 320, wsp, crfp_dsv_workspace_bytes(3, 180, 320), stream) == 0);
        EXPECT(crfp_debug_side_tables() >= 1);
        EXPECT(crfp_shutdown() == 0);
        EXPECT(crfp_dsv_forward_clip(pk, 0, lrs, fvs, mks, out, 2, 20, 36, wsp, crfp_dsv_workspace_bytes(2, 20, 36), stream) == 0);   // and a fresh call after it
        std::printf("host_check: %ld launches enqueued on the stub runtime\n", crfp_stub_launches() - l0);
    }
    // ---- the fused DCN launch with a warp plan in its idle last-round CUs (crfp_dcn_tail_probe): the argument block and the grid sizing on the
    // stub's 256 CUs -- fewer tiles than CUs, a multiple of the CUs (no plan: the stand-alone warp), one tile more than a multiple, the persistent form
    {
        crfp_dcn_tail_args a;
        std::memset(&a, 0, sizeof(a));
        crfp_dcn_tail_report r;
        void* const p = reinterpret_cast<void*>(256);
        a.feat = a.flow = a.wconv = a.bconv = a.x = a.wdcn = a.bdcn = a.warp_src = a.warp_flow = p;
        a.out = a.warp_dst = p;
        a.status = reinterpret_cast<unsigned*>(256);
        struct Shape { int n, h, w, tiles, wgs, persistent; };
        const Shape shapes[] = {{1, 20, 36, 6, 250, 0},    {1, 33, 47, 10, 246, 0},  {2, 33, 47, 20, 236, 0}, {1, 128, 544, 272, 240, 0}, {4, 64, 256, 256, 0, 0},
                                {1, 64, 257, 72, 184, 0},  {4, 64, 288, 288, 224, 0}, {1, 8, 8192, 256, 0, 0}, {1, 8, 8192 + 32, 257, 255, 0},
                                {1, 360, 640, 900, 124, 0}, {2, 360, 640, 1800, 0, 1}, {1, 384, 1024, 1536, 0, 1}, {1, 383, 1024, 1536, 0, 1}, {1, 376, 1024, 1504, 32, 0}};
        for (const Shape& sh : shapes)
            for (int bands = 0; bands <= 3; ++bands) {
                a.n = sh.n; a.h = sh.h; a.w = sh.w; a.bands = bands;
                EXPECT(crfp_dcn_tail_plan(&a, &r) == 0 && crfp_dcn_tail_plan_bf16(&a, &r) == 0);
                EXPECT(r.cus == 256 && r.tiles == sh.tiles && r.warp_wgs == sh.wgs && r.persistent == sh.persistent);
                const bool taken = bands > 0 && sh.wgs > 0;
                EXPECT(r.plan_taken == taken && r.grid == (sh.persistent ? 256 : sh.tiles + (taken ? sh.wgs : 0)));
                EXPECT(!taken || (r.tiles + r.warp_wgs) % 256 == 0);   // the plan's workgroups fill the last round exactly
                for (int bf = 0; bf < 2; ++bf) {
                    const long l0 = crfp_stub_launches();
                    crfp_dcn_tail_report q;
                    EXPECT((bf ? crfp_dcn_tail_probe_bf16 : crfp_dcn_tail_probe)(&a, &q, nullptr) == 0 && std::memcmp(&q, &r, sizeof(q)) == 0);
                    EXPECT(crfp_stub_launches() == l0 + (taken ? bands : 2));   // k fused launches, or the fused launch and the stand-alone warp
                    if (taken) EXPECT(crfp_stub_last_grid(0) == r.grid && crfp_stub_last_grid(1) == 1 && crfp_stub_last_grid(2) == 1 && crfp_stub_last_grid(3) == 512);
                    else EXPECT(crfp_stub_last_grid(0) == (4 * sh.w + 63) / 64 && crfp_stub_last_grid(1) == sh.h && crfp_stub_last_grid(2) == sh.n);
                }
            }
        // refusals, before any launch
        const long l0 = crfp_stub_launches();
        a.n = 1; a.h = 20; a.w = 36; a.bands = 4;
        EXPECT(crfp_dcn_tail_plan(&a, &r) == CRFP_E_BADARG && crfp_dcn_tail_probe(&a, &r, nullptr) == CRFP_E_BADARG);
        a.bands = 3; a.h = 0;
        EXPECT(crfp_dcn_tail_probe_bf16(&a, &r, nullptr) == CRFP_E_BADARG);
        a.h = 20; a.warp_dst = nullptr;
        EXPECT(crfp_dcn_tail_probe(&a, &r, nullptr) == CRFP_E_BADARG && std::strstr(crfp_last_error_string(), "null tensor") != nullptr);
        a.warp_dst = p;
        EXPECT(crfp_dcn_tail_probe(&a, nullptr, nullptr) == CRFP_E_BADARG && crfp_dcn_tail_plan(nullptr, &r) == CRFP_E_BADARG);
        EXPECT(crfp_stub_launches() == l0);
    }
    // ---- one gather launch at a time (crfp_gather_probe): every mode in both builds on the stub runtime -- the workspace layout, the plan items
    // and the launch arguments under the sanitizers -- the report on the stub's 256 CUs, and the refusals, which come before any launch
    {
        crfp_gather_args a;
        std::memset(&a, 0, sizeof(a));
        crfp_gather_report r, q;
        float* const p = reinterpret_cast<float*>(256);
        void* const wsp = reinterpret_cast<char*>(1ull << 40);
        a.x = a.x2 = a.aux = a.mask = a.flow = a.head_w = a.head_b = a.weight = a.bias = p;
        a.out = a.out2 = p;
        a.status = reinterpret_cast<unsigned*>(256);
        static const int kernels[6] = {CRFP_GATHERK_WARP_P4, CRFP_GATHERK_WARP_DUAL_SPLIT, CRFP_GATHERK_DCN_G8_PIPE, CRFP_GATHERK_DCN_FUSED, CRFP_GATHERK_DCN3,
                                       CRFP_GATHERK_DCN3_FUSED};
        for (int mode = CRFP_GPROBE_WARP; mode <= CRFP_GPROBE_DCN3_FUSED; ++mode)
            for (int bf = 0; bf < 2; ++bf) {
                a.mode = mode; a.c = 24; a.n = 3; a.h = 9; a.w = 33;
                const size_t bytes = (bf ? crfp_gather_probe_workspace_bytes_bf16 : crfp_gather_probe_workspace_bytes)(&a);
                EXPECT(bytes > 0);
                EXPECT((bf ? crfp_gather_probe_plan_bf16 : crfp_gather_probe_plan)(&a, &r) == 0 && r.kernel == kernels[mode]);
                EXPECT(r.out_stride > (mode == CRFP_GPROBE_WARP ? 24 : (mode >= CRFP_GPROBE_DCN3 ? 4 : 32)) * 9 * 33 && (mode == CRFP_GPROBE_WARP_DUAL) == (r.out2_stride > 0));
                if (mode == CRFP_GPROBE_DCN_FUSED) EXPECT(r.cus == 256 && r.tiles == 3 * 2 * 2 && !r.persistent);
                const long l0 = crfp_stub_launches();
                EXPECT((bf ? crfp_gather_probe_bf16 : crfp_gather_probe)(&a, &q, wsp, bytes, nullptr) == 0 && std::memcmp(&q, &r, sizeof(q)) == 0);
                EXPECT(crfp_stub_launches() > l0);
                EXPECT((bf ? crfp_gather_probe_bf16 : crfp_gather_probe)(&a, &q, wsp, bytes - 1, nullptr) == CRFP_E_WORKSPACE);
                EXPECT((bf ? crfp_gather_probe_bf16 : crfp_gather_probe)(&a, &q, nullptr, bytes, nullptr) == CRFP_E_WORKSPACE);
            }
        // the launchers' own choices: the unsplit dual warp past 65 535 z groups, the persistent fused form from 6 rounds of the chip
        a.mode = CRFP_GPROBE_WARP_DUAL; a.n = 16384; a.h = 1; a.w = 2;
        EXPECT(crfp_gather_probe_plan(&a, &r) == 0 && r.kernel == CRFP_GATHERK_WARP_DUAL && !r.split);
        a.n = 16383;
        EXPECT(crfp_gather_probe_plan_bf16(&a, &r) == 0 && r.kernel == CRFP_GATHERK_WARP_DUAL_SPLIT && r.split);
        a.mode = CRFP_GPROBE_DCN_FUSED; a.n = 1537; a.h = 3; a.w = 5;
        EXPECT(crfp_gather_probe_plan(&a, &r) == 0 && r.kernel == CRFP_GATHERK_DCN_FUSED_PS && r.persistent && r.tiles == 1537);
        a.n = 1535;
        EXPECT(crfp_gather_probe_plan_bf16(&a, &r) == 0 && r.kernel == CRFP_GATHERK_DCN_FUSED && !r.persistent);
        // refusals
        const long l0 = crfp_stub_launches();
        auto refused = [&](int rc, const char* text) {
            const bool f32 = crfp_gather_probe_workspace_bytes(&a) == 0 && std::strstr(crfp_last_error_string(), text) != nullptr && crfp_gather_probe_plan(&a, &r) == rc;
            const bool b16 = crfp_gather_probe_workspace_bytes_bf16(&a) == 0 && std::strstr(crfp_last_error_string(), text) != nullptr && crfp_gather_probe_plan_bf16(&a, &r) == rc;
            return f32 && b16 && crfp_gather_probe(&a, &r, wsp, 1 << 20, nullptr) == rc && crfp_gather_probe_bf16(&a, &r, wsp, 1 << 20, nullptr) == rc;
        };
        a.n = 3; a.h = 9; a.w = 33;
        a.mode = 6;
        EXPECT(refused(CRFP_E_BADARG, "unknown mode 6"));
        a.mode = CRFP_GPROBE_WARP; a.c = 8;
        EXPECT(refused(CRFP_E_BADARG, "a warp takes 4, 24 or 32 channels"));
        a.c = 4; a.n = 0;
        EXPECT(refused(CRFP_E_BADARG, "bad geometry (n=0 h=9 w=33)"));
        a.n = 65536;
        EXPECT(refused(CRFP_E_BADARG, "bad geometry"));
        a.n = 1; a.w = 0;
        EXPECT(refused(CRFP_E_BADARG, "bad geometry"));
        a.h = 2047; a.w = 2047;
        EXPECT(refused(CRFP_E_UNSUPPORTED, "plane of 2047 x 2047 exceeds the hook's 2^22-element range"));
        a.mode = CRFP_GPROBE_DCN_G8;
        EXPECT(refused(CRFP_E_UNSUPPORTED, "plane of 2047 x 2047 exceeds the hook's 2^22-element range"));
        a.h = 2047; a.w = 2046; a.n = 1;   // just inside: sized, never launched here
        EXPECT(crfp_gather_probe_workspace_bytes(&a) > 0 && crfp_gather_probe_plan_bf16(&a, &r) == 0);
        a.n = 3;
        a.h = 9; a.w = 33;
        EXPECT(crfp_gather_probe_workspace_bytes(nullptr) == 0 && crfp_gather_probe_plan_bf16(nullptr, &r) == CRFP_E_BADARG && crfp_gather_probe_plan(&a, nullptr) == CRFP_E_BADARG);
        EXPECT(crfp_gather_probe(&a, nullptr, wsp, 1 << 20, nullptr) == CRFP_E_BADARG);
        // null tensors, per mode: what the mode reads, and nothing it does not
        struct Null { int mode; const float** field; const char* text; };
        const Null nulls[] = {{CRFP_GPROBE_WARP, &a.x, "null tensor"}, {CRFP_GPROBE_WARP, &a.flow, "null tensor"}, {CRFP_GPROBE_WARP_DUAL, &a.x2, "null tensor"},
                              {CRFP_GPROBE_DCN_G8, &a.aux, "null tensor"}, {CRFP_GPROBE_DCN_G8, &a.mask, "null tensor"}, {CRFP_GPROBE_DCN_G8, &a.weight, "null weight or bias"},
                              {CRFP_GPROBE_DCN_FUSED, &a.flow, "null tensor"}, {CRFP_GPROBE_DCN_FUSED, &a.head_w, "null head weight or bias"},
                              {CRFP_GPROBE_DCN3, &a.bias, "null weight or bias"}, {CRFP_GPROBE_DCN3_FUSED, &a.head_b, "null head weight or bias"}};
        for (const Null& z : nulls) {
            a.mode = z.mode;
            *z.field = nullptr;
            const size_t bytes = crfp_gather_probe_workspace_bytes(&a);   // sizes do not ask for tensors
            EXPECT(bytes > 0 && crfp_gather_probe(&a, &r, wsp, bytes, nullptr) == CRFP_E_BADARG && std::strstr(crfp_last_error_string(), z.text) != nullptr);
            EXPECT(crfp_gather_probe_bf16(&a, &r, wsp, bytes, nullptr) == CRFP_E_BADARG);
            *z.field = p;
        }
        a.mode = CRFP_GPROBE_DCN3; a.mask = a.flow = a.head_w = a.x2 = nullptr;   // ... dcn3 reads none of these
        EXPECT(crfp_stub_launches() == l0);
        EXPECT(crfp_gather_probe(&a, &r, wsp, crfp_gather_probe_workspace_bytes(&a), nullptr) == 0 && crfp_stub_launches() > l0);
    }
    std::printf("host_check: %d parameters (dsv) / %d (cra) / %d (rt), %d failed expectations\n", np, nc, nr, fails);
    return fails ? 1 : 0;
}
