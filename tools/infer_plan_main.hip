// Stand-alone host program: plan_model (unmicst_amd/csrc/umx_plan.hip) on three graphs of the inference engine, for a sanitizer run of
// the planner outside Python.  No device is used and the engine is not linked.  From the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/infer_plan_main.hip unmicst_amd/csrc/{umx_plan,umx_graph,umx_kernels,umx_conv_first}.hip -o /tmp/infer_plan_main && /tmp/infer_plan_main
// It prints each launch's plan lines, kernel, digest and the launch_shape at batches 5 and 278, and exits 0; a refusal it does not
// expect, or a sanitizer report, is a failure.
#include "../unmicst_amd/csrc/umx_internal.h"

using namespace umx;

namespace umx {
thread_local std::string g_err;   // (umx_engine.hip is not linked)
int fail(umx_ctx*, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
}  // namespace umx

static int run(const char* what, const umx_hparams& hp, const PlanSwitches& sw) {
    printf("-- %s\n", what);
    std::string why;
    if (check_hp(&hp, &why)) { printf("bad hyper-parameters: %s\n", why.c_str()); return 1; }
    std::vector<float> blob(blob_floats_needed(hp));   // positive everywhere: a BN variance among them stays one
    for (size_t i = 0; i < blob.size(); ++i) blob[i] = 0.01f + 0.05f * (float)(i * 2654435761u % 201) / 200.f;
    ModelPlan m;
    if (plan_model(hp, blob.data(), true, true, 0, sw, &m, &why)) { printf("refused: %s\n", why.c_str()); return 1; }
    for (size_t li = 0; li < m.plan.size(); ++li) {
        Launch& L = m.plan[li];
        if (L.head) continue;
        const HostPlan& P = m.hplans[li];
        adopt_plan(L, P);
        const LaunchShape a = launch_shape(L, P.h, 5), b = launch_shape(L, P.h, 278);
        printf("%s           %s, digest %016llx, order/tiles per XCD at 5: %d/%d, at 278: %d/%d\n", plan_describe(L, P).c_str(), L.kernel.c_str(),
               infer_digest(P), a.xcd_order, a.tiles_per_xcd, b.xcd_order, b.tiles_per_xcd);
    }
    return 0;
}

int main() {
    const umx_hparams HP = {UMX_GRAPH_V2, 64, 2, 3, 28, 3, 3, 0, 2};       // the graph of tests/test_gpu_switches.py
    const umx_hparams order2 = {UMX_GRAPH_V2, 32, 2, 3, 40, 3, 3, 0, 2};   // layers of 2 and 3 N-blocks: workgroup order 2 at 278 tiles
    int bad = run("default switches", HP, PlanSwitches());
    bad += run("UMX_PLAN_OVERRIDE=lu0.conv:3:2,ld1.conv:1:1:12", HP, plan_switches_parse(nullptr, "lu0.conv:3:2,ld1.conv:1:1:12", nullptr, false, nullptr));
    bad += run("UMX_PLAN_NT=ld0.conv:1 (no dense-K first layer: planned again without the fold)", HP, plan_switches_parse("ld0.conv:1", nullptr, nullptr, false, nullptr));
    bad += run("UMX_PLAN_NT=lu2.convT:4", HP, plan_switches_parse("lu2.convT:4", nullptr, nullptr, false, nullptr));
    bad += run("the workgroup-order graph", order2, PlanSwitches());
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
