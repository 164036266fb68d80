// Stand-alone host program: tconv_plan (unmicst_amd/csrc/umx_tconv.hip) on a few convolutions of the training step, for a sanitizer
// run of the planner outside Python.  No device is used.  From the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/tconv_plan_main.hip unmicst_amd/csrc/{umx_tconv,umx_plan,umx_graph,umx_kernels,umx_conv_first}.hip -o /tmp/tconv_plan_main && /tmp/tconv_plan_main
// It prints each plan's line and digest and exits 0; a refusal it does not expect, or a sanitizer report, is a failure.
#include "../unmicst_amd/csrc/umx_internal.h"

#include <cstdint>

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

static int run(const TConvSpec& s, const TConvEnv& env, bool expect_ok) {
    TConvPlan p;
    std::string why;
    const bool ok = tconv_plan(s, env, &p, &why);
    if (!ok) {
        printf("refused: %s\n", why.c_str());
        return expect_ok ? 1 : 0;
    }
    printf("%s; direct %d, wsh %d, packs %zu, scratch %zu, digest %016llx\n", p.text.c_str(), p.direct ? 1 : 0, p.wsh, p.packs.size(),
           p.split_floats, tconv_digest(p.cp, p.nt, p.hpix, p.packs.data(), p.packs.size(), p.split ? &p.P : nullptr));
    return expect_ok ? 0 : 1;
}

int main() {
    const int ks = 3, Cskip = 6, Cup = 12, Cin = 24;
    // one parameter vector for every spec: wt [9][Cup][Cin] at 0, w2 [9][Cskip + Cup][Cup] behind it
    const size_t o_wt = 0, o_w2 = (size_t)ks * ks * Cup * Cin, nparams = o_w2 + (size_t)ks * ks * (Cskip + Cup) * Cup;
    std::vector<float> params(nparams);
    for (size_t i = 0; i < nparams; ++i) params[i] = 0.05f * (float)((int)(i * 2654435761u % 201) - 100) / 100.f;
    const TapSet fwd = same_taps(ks, false), flp = same_taps(ks, true);
    int bad = 0;
    for (int route = 0; route < 3; ++route) {
        TConvEnv env;
        env.B = 3; env.imSize = 32; env.hconv = route != 1; env.no_ksplit = route == 2; env.params = params.data();
        {   // the four-phase transposed convolution
            TConvSpec s;
            s.name = "lu0"; s.H = s.W = 8; s.Cout = Cup; s.act = ACT_LEAKY; s.nphase = 4; s.o_mul = 2; s.ngroups = 1;
            s.g[0] = one_group(Cin, o_wt, SIZE_MAX, Cup, Cin, 1, 0, TapSet());
            transposed_fwd_taps(ks, &s.g[0], s.oy, s.ox);
            bad += run(s, env, true);
        }
        {   // its input gradient on the space-to-depth tensor: parity blocks of 12 channels, so no direct references
            TConvSpec s;
            s.name = "lu0"; s.H = s.W = 8; s.Cout = Cin; s.ngroups = 1; s.bwd = true;
            s.g[0] = one_group(4 * Cup, o_wt, SIZE_MAX, Cup, Cin, 0, 0, TapSet());
            TapSet slabs;
            std::vector<int> coff;
            transposed_bwd_taps(ks, Cup, &s.g[0], &slabs, &coff);
            bad += run(s, env, true);
        }
        {   // the two-group concat convolution at 16 x 16, and its input gradient into the skip
            TConvSpec s;
            s.name = "lu0"; s.H = s.W = 16; s.Cout = Cup; s.ngroups = 2;
            s.g[0] = one_group(Cskip, o_w2, SIZE_MAX, Cskip + Cup, Cup, 0, 0, fwd);
            s.g[1] = one_group(Cup, o_w2, SIZE_MAX, Cskip + Cup, Cup, 0, Cskip, fwd);
            bad += run(s, env, true);
            TConvSpec d;
            d.name = "lu0"; d.H = d.W = 16; d.Cout = Cskip; d.ngroups = 1; d.bwd = true;
            d.g[0] = one_group(Cup, o_w2, SIZE_MAX, Cskip + Cup, Cup, 1, 0, flp);
            bad += run(d, env, true);
        }
        {   // a 2 x 2 layer (64 images a tile, 3 in the batch), and a size that is no power of two: refused
            TConvSpec s;
            s.name = "lb"; s.H = s.W = 2; s.Cout = Cup; s.ngroups = 1;
            s.g[0] = one_group(Cup, o_w2, SIZE_MAX, Cskip + Cup, Cup, 0, 0, fwd);
            bad += run(s, env, true);
            s.H = s.W = 12;
            bad += run(s, env, false);
        }
    }
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
