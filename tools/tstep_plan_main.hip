// Stand-alone host program: step_plan (unmicst_amd/csrc/umx_tstep.hip) over the depths and routes of tests/test_step_plan_cpu.py, for a
// sanitizer run of the schedule's builder outside Python.  No device is used.  From the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/tstep_plan_main.hip unmicst_amd/csrc/umx_tstep.hip -o /tmp/tstep_plan_main && /tmp/tstep_plan_main
// It prints each plan's size and the L = 2 plans' lines and exits 0; a plan whose ids leave their ranges, or whose waits name an event no
// earlier step records, or a sanitizer report, is a failure.
#include "../unmicst_amd/csrc/umx_internal.h"

using namespace umx;

static int check(const StepEnv& env, bool print) {
    const StepPlan p = step_plan(env);
    int bad = 0;
    std::vector<char> recorded(p.nevents, 0);
    for (const TStep& s : p.steps) {
        bad += s.op >= T_NOPS || s.stream >= kStepStreams || s.site > site_top(env.L) || s.nwait > 3 || s.nrec > 2;
        bad += (size_t)s.r0 + s.nr > p.bufs.size() || (size_t)s.w0 + s.nw > p.bufs.size();
        for (int k = 0; k < s.nwait; ++k) bad += s.wait[k] >= p.nevents || !recorded[s.wait[k]];
        for (int k = 0; k < s.nrec; ++k) {
            bad += s.rec[k] >= p.nevents;
            if (s.rec[k] < p.nevents) recorded[s.rec[k]] = 1;
        }
        for (int k = 0; k < s.nr; ++k) bad += p.rd(s, k) / 32 >= TB_NKINDS;
        for (int k = 0; k < s.nw; ++k) bad += p.wr(s, k) / 32 >= TB_NKINDS;
    }
    const std::string text = step_describe(p);
    printf("L %d hconv %d reg %d: %zu steps, %d events, %zu buffer references, %zu bytes of text%s\n", env.L, env.hconv ? 1 : 0,
           env.reg ? 1 : 0, p.steps.size(), p.nevents, p.bufs.size(), text.size(), bad ? " -- BAD" : "");
    if (print) printf("%s", text.c_str());
    return bad;
}

int main() {
    int bad = 0;
    for (int L : {1, 2, 3, 5, 8})
        for (int route = 0; route < 3; ++route)      // split precision everywhere | the exact-fp32 route | every second convolution refused
            for (int reg = 0; reg < 2; ++reg) {
                StepEnv env;
                env.L = L; env.hconv = route != 1; env.wg_planes = env.hconv; env.reg = reg != 0;
                for (int idx = 0; idx < L; ++idx) env.skip_split[idx] = env.T_split[idx] = env.hconv && (route == 0 || idx % 2 == 1);
                bad += check(env, L == 2 && reg);
            }
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
