// libumx training step: the host plan of one forward / input-gradient convolution (umx_internal.h: TConvSpec, TConvEnv -> TConvPlan).
//
// Everything here runs on the host: no HIP call, no trainer, no environment variable.  tconv_plan decides what umx_train.hip's
// upload_conv then allocates and sends -- the fp32 kernel's geometry and pack descriptors, the split-precision plan with its weight
// references already in the coordinates the per-step repack reads, both K-split rules and the scratch they need -- so a plan can be
// read, diffed and tested without a device (umx_test_train_plan, tests/test_tconv_plan_cpu.py).
#include "umx_internal.h"
#include "umx_kernels.h"

#include <climits>
#include <cmath>

namespace umx {

TapSet same_taps(int ks, bool flipped) {   // stride-1 SAME conv (or its input gradient: offsets negated)
    TapSet t;
    const int ph = (ks - 1) / 2;
    for (int a = 0; a < ks; ++a)
        for (int b = 0; b < ks; ++b) {
            t.off.push_back(flipped ? std::make_pair(ph - a, ph - b) : std::make_pair(a - ph, b - ph));
            t.m.push_back(a * ks + b);
        }
    return t;
}

// a single-phase group of one source: C channels, master tensor(s) at w_off (+ w2_off) of dims [taps][d2][d3]
GroupSpec one_group(int C, size_t w_off, size_t w2_off, int d2, int d3, int transpose, int c_off, const TapSet& ts) {
    GroupSpec g;
    g.C = C; g.w_off = w_off; g.w2_off = w2_off; g.d2 = d2; g.d3 = d3; g.transpose = transpose; g.c_off = c_off;
    g.npar = 1; g.Cblk = std::max(C, 1);
    g.taps[0] = ts;
    return g;
}

// transposed conv forward: 4 sub-pixel phases (out[2i+a-pb] += in[i] * Wt[a])
void transposed_fwd_taps(int ks, GroupSpec* g, int* oy, int* ox) {
    const int pb = (ks - 2) / 2;   // pad_before of the stride-2 SAME conv whose gradient the transposed conv is
    for (int p = 0; p < 4; ++p) {
        const int pu = p >> 1, pv = p & 1;
        oy[p] = pu; ox[p] = pv;
        for (int a = 0; a < ks; ++a) {
            if (((a - pb - pu) & 1) != 0) continue;
            for (int b = 0; b < ks; ++b) {
                if (((b - pb - pv) & 1) != 0) continue;
                g->taps[p].off.push_back({(pu + pb - a) / 2, (pv + pb - b) / 2});
                g->taps[p].m.push_back(a * ks + b);
            }
        }
    }
}

// transposed conv backward on the space-to-depth gradient gS[.., (pa,pb)*Cup + c] = dY[2i+pa, 2j+pb, c]:
// dX[i] = sum_a dY[2i + a - pb] Wt[a]  ->  q = a - pb = 2*di + pa
void transposed_bwd_taps(int ks, int Cup, GroupSpec* g, TapSet* slabs, std::vector<int>* coff) {
    const int pb = (ks - 2) / 2;
    auto split = [](int q, int* d, int* par) { *par = ((q % 2) + 2) % 2; *d = (q - *par) / 2; };
    std::vector<std::pair<int, int>> offs;
    for (int a = 0; a < ks; ++a)
        for (int b = 0; b < ks; ++b) {
            int di, pa, dj, pbb;
            split(a - pb, &di, &pa);
            split(b - pb, &dj, &pbb);
            std::pair<int, int> od{di, dj};
            if (std::find(offs.begin(), offs.end(), od) == offs.end()) offs.push_back(od);
        }
    g->npar = 4; g->Cblk = Cup;
    g->taps[0].off = offs;
    g->taps[0].m.assign(offs.size() * 4, -1);
    for (int par = 0; par < 4; ++par)   // weight-gradient slabs, grouped by parity block
        for (int a = 0; a < ks; ++a)
            for (int b = 0; b < ks; ++b) {
                int di, pa, dj, pbb;
                split(a - pb, &di, &pa);
                split(b - pb, &dj, &pbb);
                if (pa * 2 + pbb != par) continue;
                const size_t t = std::find(offs.begin(), offs.end(), std::make_pair(di, dj)) - offs.begin();
                g->taps[0].m[t * 4 + par] = a * ks + b;
                slabs->off.push_back({di, dj});
                slabs->m.push_back(a * ks + b);
                coff->push_back(par * Cup);
            }
}

// N-tiles per workgroup.  A training batch is small (8 images): the deep layers have a handful of 256-pixel M-tiles, so
// wide N blocks would leave most of the 256 CUs idle.  Cost model: rounds of 512 resident workgroups (2 per CU) times
// the work of one workgroup (NT MFMAs per fragment pair + a fixed staging share); padded N counts as work.
void choose_nt(int Cout, int mtiles, int* nt, int* Np) {
    const int t16 = (Cout + 15) / 16;
    int best = 1;
    double best_cost = 1e300;
    for (int c = 1; c <= kMaxNT; ++c) {
        const long wgs = (long)mtiles * ((t16 + c - 1) / c);
        const double cost = (double)((wgs + 511) / 512) * (c + 0.5);
        if (cost < best_cost - 1e-9 || (std::fabs(cost - best_cost) <= 1e-9 && c > best)) { best = c; best_cost = cost; }
    }
    *nt = best;
    *Np = round_up(t16, best) * 16;
}

// largest |w| a convolution's packed operand can hold: the master tensor(s) each group reads (a summed pair: the sum of the maxima)
double operand_wmax(const std::vector<WSrc>& wsrc, const float* params) {
    double wmax = 0.0;
    for (const WSrc& w : wsrc) {
        double m1 = 0.0, m2 = 0.0;
        for (size_t i = 0; i < w.cnt; ++i) m1 = std::max(m1, (double)std::fabs(params[w.off + i]));
        if (w.off2 != SIZE_MAX)
            for (size_t i = 0; i < w.cnt; ++i) m2 = std::max(m2, (double)std::fabs(params[w.off2 + i]));
        wmax = std::max(wmax, m1 + m2);
    }
    return wmax;
}
// s such that wmax * 2^s is in [2^10, 2^11): 32 x headroom below binary16's largest finite value for the weights to grow into
int wscale_shift(double wmax) {
    if (!(wmax > 0.0) || !std::isfinite(wmax)) return 0;
    int e;
    std::frexp(wmax, &e);              // wmax = m * 2^e, m in [0.5, 1)
    return std::max(-24, std::min(40, 11 - e));
}

namespace {

bool refuse(std::string* why, const TConvSpec& s, const std::string& msg) {
    *why = s.name + ": " + msg;
    return false;
}

// Geometry + pack descriptors of the launch on conv_mfma_f32 (every convolution has them: the kernel of the exact-fp32 route, and of
// a shape the split-precision planner refuses)
bool plan_f32(const TConvSpec& s, const TConvEnv& env, TConvPlan* out, std::string* why) {
    const int H = s.H, W = s.W, Cout = s.Cout, nphase = s.nphase, ngroups = s.ngroups;
    ConvParams& p = out->cp;
    memset(&p, 0, sizeof p);
    {
        const int TWm0 = std::min(16, W), TH0 = std::min(16, H);
        const int imgs0 = (16 / TWm0) * (16 / TH0);
        choose_nt(Cout, ((env.B + imgs0 - 1) / imgs0) * (H / TH0) * (W / TWm0) * nphase, &out->nt, &p.Np);
    }
    int ymin = 0, ymax = 0, xmin = 0, xmax = 0, ntaps_total = 0;
    for (int g = 0; g < ngroups; ++g)
        for (int ph = 0; ph < nphase; ++ph)
            for (auto& t : s.g[g].taps[ph].off) {
                ymin = std::min(ymin, t.first); ymax = std::max(ymax, t.first);
                xmin = std::min(xmin, t.second); xmax = std::max(xmax, t.second);
                ++ntaps_total;
            }
    if (ntaps_total > kMaxTaps) return refuse(why, s, "too many filter taps");
    auto lg2 = [](int v) { int l = 0; while ((1 << l) < v) ++l; return l; };
    const int TWm = std::min(16, W), TH = std::min(16, H);
    if ((TWm & (TWm - 1)) || (TH & (TH - 1))) return refuse(why, s, "layer size " + std::to_string(H) + " must be a power of two");
    p.twm_log2 = lg2(TWm);
    p.th_log2 = lg2(TH);
    p.nimg_m = 16 / TWm;
    p.imgs = p.nimg_m * (16 / TH);
    p.hh = TH + ymax - ymin;
    p.hw = TWm + xmax - xmin;
    p.imgplane = p.hh * p.hw;
    int plane = round_up(p.imgs * p.imgplane, 32) + 16;
    if (plane - 32 >= p.imgs * p.imgplane) plane -= 32;
    p.plane = plane;
    p.ymin = ymin;
    p.xmin = xmin;
    p.tiles_y = H / TH;
    p.tiles_x = W / TWm;
    out->hpix = (p.imgs * p.imgplane + 255) / 256;
    if (out->hpix > 4) return refuse(why, s, "halo too large");
    out->hpix = out->hpix <= 2 ? 2 : 4;
    p.ngroups = ngroups;
    p.H = H; p.W = W; p.Cout = Cout;
    p.nphase = nphase; p.o_mul = s.o_mul;
    p.outH = H * s.o_mul; p.outW = W * s.o_mul; p.pool = 0; p.act = s.act;
    {   // K split: a deep layer of a small batch has a few dozen workgroups, each walking thousands of K steps with
        // exposed staging latency -- spread the channel chunks over more workgroups (partials + ordered reduce)
        const int img_groups = (env.B + p.imgs - 1) / p.imgs;
        const long wgs = (long)img_groups * p.tiles_y * p.tiles_x * nphase * (p.Np / 16 / out->nt);
        int min_chunks = 1 << 30;
        for (int g = 0; g < ngroups; ++g) min_chunks = std::min(min_chunks, (round_up(s.g[g].C, 4) + kCC - 1) / kCC);
        int S = 1;
        const long target = 1536, smax = 8;
        if (wgs < target / 2 && !env.no_ksplit)
            S = (int)std::max<long>(1, std::min<long>(std::min<long>(smax, target / wgs), min_chunks / 4));
        p.ksplit = S;
        p.split_stride = (size_t)env.B * p.outH * p.outW * Cout;
        if (S > 1) out->split_floats = std::max(out->split_floats, (size_t)S * p.split_stride);
    }
    if (conv_lds_bytes(out->nt, p.plane) > 160 * 1024) return refuse(why, s, "LDS footprint too large");
    int tpos = 0;
    for (int ph = 0; ph < nphase; ++ph) {
        p.ph[ph].oy_off = s.oy[ph];
        p.ph[ph].ox_off = s.ox[ph];
        for (int g = 0; g < ngroups; ++g) {
            const TapSet& ts = s.g[g].taps[ph];
            p.ph[ph].tap0[g] = tpos;
            p.ph[ph].ntaps[g] = (int)ts.off.size();
            for (auto& t : ts.off) p.tapoff[tpos++] = (short)((t.first - ymin) * p.hw + (t.second - xmin));
        }
    }
    for (int g = 0; g < ngroups; ++g) {
        p.C[g] = s.g[g].C;
        p.Cp[g] = round_up(s.g[g].C, 4);
        p.vec4[g] = (s.g[g].C % 4) == 0;
    }
    // packed operands + descriptors
    for (int ph = 0; ph < nphase; ++ph)
        for (int g = 0; g < ngroups; ++g) {
            const GroupSpec& G = s.g[g];
            const TapSet& ts = G.taps[ph];
            const int nt = (int)ts.off.size();
            if (nt == 0) continue;
            if (nt * G.npar > 4 * kMaxPackTaps) return refuse(why, s, "too many taps to pack");
            PackDesc d;
            memset(&d, 0, sizeof d);
            d.ntaps = nt; d.Cp = p.Cp[g]; d.Np = p.Np; d.C = G.C; d.N = Cout;
            d.d2 = G.d2; d.d3 = G.d3;
            d.transpose = G.transpose; d.c_off = G.c_off;
            d.npar = G.npar; d.Cblk = G.Cblk;
            for (size_t i = 0; i < ts.m.size(); ++i) d.mtap[i] = (short)ts.m[i];
            d.bwd = s.bwd ? 1 : 0;
            out->operands.push_back({ph, g, (size_t)nt * p.Cp[g] * p.Np});
            out->packs.push_back(d);
            out->mac += (double)H * W * nt * G.C * Cout;
        }
    return true;
}

// The same convolution as a split-precision plan (conv_f16x3, fp32 output): stage tables and the LDS-image layout of the weights
// come from plan_f16 once; the values are filled every step by repack_f16x3_kernel.  False (with *why) where the planner refuses the
// shape -- it stays on the fp32 kernel -- and, with *fatal, where the trainer cannot take it at all.
bool plan_split(const TConvSpec& s, const TConvEnv& env, TConvPlan* out, std::string* why, bool* fatal) {
    const int nphase = s.nphase, ngroups = s.ngroups;
    Launch L;
    L.name = s.name;
    L.train = true;
    L.ngroups = ngroups; L.nphase = nphase; L.o_mul = s.o_mul;
    for (int ph = 0; ph < nphase; ++ph) { L.oy_off[ph] = s.oy[ph]; L.ox_off[ph] = s.ox[ph]; }
    L.H = s.H; L.W = s.W; L.Cout = s.Cout; L.outH = s.H * s.o_mul; L.outW = s.W * s.o_mul; L.pool = 0; L.act = s.act; L.dst = -1;
    L.Np = out->cp.Np;
    for (int g = 0; g < ngroups; ++g) {
        const GroupSpec& G = s.g[g];
        L.g[g].src = g;
        L.g[g].C = G.C;
        for (int ph = 0; ph < nphase; ++ph) L.g[g].taps[ph] = G.taps[ph].off;
        if (G.npar > 1 && G.Cblk % 8 == 0) {
            const int noct = (G.C + 7) / 8;
            for (int ph = 0; ph < nphase; ++ph) {
                const TapSet& ts = G.taps[ph];
                L.g[g].dead[ph].assign(ts.off.size() * (size_t)noct, 0);
                for (size_t t = 0; t < ts.off.size(); ++t)
                    for (int o = 0; o < noct; ++o)
                        if (ts.m[t * G.npar + (size_t)(8 * o / G.Cblk)] < 0) L.g[g].dead[ph][t * noct + o] = 1;
            }
        }
        // the master tensor(s) this group reads: where the largest |w| the packed operand can hold is taken from
        int ntap_master = 0;
        for (int ph = 0; ph < nphase; ++ph)
            for (int m : G.taps[ph].m) ntap_master = std::max(ntap_master, m + 1);
        out->wsrc.push_back({G.w_off, G.w2_off, (size_t)ntap_master * G.d2 * G.d3});
    }
    PlanInputs in;
    in.imSize = env.imSize;
    in.out_f32 = true;
    in.sw = env.sw;
    HostPlan& P = out->P;
    if (!conv_geometry(L, why) || plan_f16(L, in, &P, why) != UMX_OK) return false;
    if (env.sw.debug_plan) fputs(plan_describe(L, P).c_str(), stderr);
    HConvParams& h = P.h;   // (the weight slabs hold the k-maps; repack_f16x3_kernel writes their values every step)
    out->wsh = wscale_shift(operand_wmax(out->wsrc, env.params));
    static_assert(sizeof(HWRef) == sizeof(HWRefDev) && sizeof(HWRefDev) == 12, "reference record layout");
    // The planner's references address the packed fp32 operand [tap][Cp][Np]; rewritten here into the master tensor's own
    // coordinates (the index arithmetic of pack_weights_kernel, done once on the host), the per-step repack reads the parameters
    // directly and this convolution needs no fp32 operand at all.  An octet that straddles two parity blocks keeps the packed route.
    bool direct = true;
    for (int ph = 0; ph < nphase && direct; ++ph)
        for (const HWRef& r : P.wrefs[ph]) {
            const GroupSpec& G = s.g[r.arr];
            const int c0 = (int)(((size_t)r.base / L.Np) % round_up(G.C, 4));
            if (c0 / G.Cblk != (c0 + r.nvalid - 1) / G.Cblk) { direct = false; break; }
        }
    if (direct)
        for (int ph = 0; ph < nphase; ++ph) {
            std::vector<HWRef> refs;
            refs.reserve(P.wrefs[ph].size());
            for (const HWRef& r : P.wrefs[ph]) {
                const GroupSpec& G = s.g[r.arr];
                const int Cp = round_up(G.C, 4);
                const int co = (int)((size_t)r.base % L.Np);
                const size_t row = (size_t)r.base / L.Np;
                const int c0 = (int)(row % Cp), t = (int)(row / Cp);
                const int par = c0 / G.Cblk, cc = c0 - par * G.Cblk;
                const int m = G.taps[ph].m[(size_t)t * G.npar + par];
                if (m < 0) continue;   // a tap this parity block does not have: the unit stays zero
                const size_t idx = G.transpose ? ((size_t)m * G.d2 + G.c_off + co) * G.d3 + cc : ((size_t)m * G.d2 + G.c_off + cc) * G.d3 + co;
                if (idx > (size_t)INT_MAX) {
                    *fatal = true;
                    return refuse(why, s, "master tensor too large for a weight reference");
                }
                refs.push_back(HWRef{r.dst, (int)idx, r.nvalid, r.arr});
            }
            P.wrefs[ph].swap(refs);
        }
    out->direct = direct;
    if (direct) out->packs.clear();   // nothing reads this convolution's fp32 operands
    // K split: enough workgroups to occupy the chip (two per CU) where a batch of 8 leaves a deep layer a few dozen
    const long wgs = (long)((env.B + h.imgs - 1) / h.imgs) * h.tiles_y * h.tiles_x * h.nblocks * nphase;
    // (one workgroup per CU: 512 / 768 / 1024 lose 3 / 7 / 10 % of the step to the ordered reduce over more partial sums, 128 / 192
    // lose 1 % to idle CUs -- profiles/r04/train_ksplit_sweep.txt)
    const long target = 256;
    int S = (int)std::min<long>(kMaxKSplit, wgs > 0 ? (target + wgs - 1) / wgs : 1);
    if (env.no_ksplit || wgs * 2 > target) S = 1;
    std::vector<std::vector<int>> starts(nphase);   // per phase: stage indices (relative) where a halo chunk begins
    for (int ph = 0; ph < nphase && S > 1; ++ph) {
        for (int si = 0; si < h.ph[ph].nstages; ++si)
            if (P.stages[h.ph[ph].stage0 + si].group >= 0) starts[ph].push_back(si);
        S = std::min(S, (int)starts[ph].size());
    }
    if (S > 1) {
        for (int ph = 0; ph < nphase; ++ph) {
            const int nch = (int)starts[ph].size();
            for (int k = 0; k < S; ++k) h.ks0[ph][k] = (short)starts[ph][(size_t)((long)nch * k / S)];
            h.ks0[ph][S] = (short)h.ph[ph].nstages;
        }
        h.ksplit = S;
        h.split_stride = (size_t)env.B * L.outH * L.outW * s.Cout;
        if (h.xcd_order == 2) h.xcd_order = 1;
        out->split_floats = std::max(out->split_floats, (size_t)S * h.split_stride);
    }
    return true;
}

}  // namespace

bool tconv_plan(const TConvSpec& s, const TConvEnv& env, TConvPlan* out, std::string* why) {
    *out = TConvPlan();
    if (!plan_f32(s, env, out, why)) return false;
    for (const TConvPlan::Operand& o : out->operands) out->max_pack = std::max(out->max_pack, o.elems);
    if (env.hconv) {
        bool fatal = false;
        out->split = plan_split(s, env, out, &out->refused, &fatal);
        if (fatal) { *why = out->refused; return false; }
        if (!out->split) out->P = HostPlan();
    }
    out->text = tconv_describe(s, env, *out);
    return true;
}

std::string tconv_describe(const TConvSpec& s, const TConvEnv& env, const TConvPlan& p) {
    char buf[512];
    if (p.split) {
        const HConvParams& h = p.P.h;
        const long wgs = (long)((env.B + h.imgs - 1) / h.imgs) * h.tiles_y * h.tiles_x * h.nblocks * s.nphase;
        snprintf(buf, sizeof buf, "%s%s: %d x %d -> %d ch, %d phase(s), NT %d x %d blocks, %d k-steps, %ld workgroups, K split %d",
                 s.name.c_str(), s.bwd ? " (backward)" : "", s.H, s.W, s.Cout, s.nphase, h.NT, h.nblocks, p.P.n_ksteps, wgs,
                 std::max(1, h.ksplit));
    } else {
        const ConvParams& c = p.cp;
        snprintf(buf, sizeof buf, "%s%s: fp32 conv, %d x %d -> %d ch, %d phase(s), NT %d, %d img/group, %ld workgroups, K split %d",
                 s.name.c_str(), s.bwd ? " (backward)" : "", s.H, s.W, s.Cout, s.nphase, p.nt, c.imgs,
                 (long)((env.B + c.imgs - 1) / c.imgs) * c.tiles_y * c.tiles_x * s.nphase * (c.Np / 16 / p.nt), c.ksplit);
    }
    return buf;
}

// ---- what the upload would send, as one 64-bit FNV-1a digest.  Serialisation (every integer as its 8-byte little-endian two's
// complement value, a float as its 4 bytes; pointers and fields the run path sets -- B, sources, destinations -- are left out):
//   ConvParams   nt hpix C[2] Cp[2] vec4[2] ngroups H W Cout Np twm_log2 th_log2 nimg_m imgs hh hw imgplane plane ymin xmin tiles_y
//                tiles_x nphase o_mul, per phase (4) tap0[2] ntaps[2] oy_off ox_off, tapoff[kMaxTaps], outH outW pool act ksplit split_stride
//   PackDesc     the count, then each: ntaps Cp Np C N d2 d3 transpose c_off npar Cblk bwd mtap[4 * kMaxPackTaps]
//   split plan   1 (else 0 and nothing more), then
//   HConvParams  dst_planar H W Cout Cds NT nblocks twm_log2 th_log2 nimg_m imgs hh hw imgplane nhalo plane_slots OC pix_bytes slot_bytes
//                inv_OC PP nact ninst piece_bytes inv_oc_q16 kmt xcd_order ntiles_grid tiles_per_xcd maxp lo_off b_off lds_bytes wbuf_bytes
//                ymin xmin tiles_y tiles_x nphase o_mul fused_phases, per phase (4) wblk_stride stage0 nstages oy_off ox_off, app_cw app_oct
//                app_word head_K outH outW pool inv_imgplane inv_hw act post_affine d2s d2s_mix f6 pk ksplit ks0[4][kMaxKSplit + 1]
//                split_stride
//   stage table  the count, then each: woff group oct0 noct nk plane0 phase
//   wimg         per phase (4): the count of halves, then their bytes
//   econst       the count, then the floats' bytes
//   HWRef        per phase (4): the count, then each: dst base nvalid arr
// From HConvParams on this is digest_host_plan (umx_plan.hip), which the inference digest shares: infer_digest is that part alone,
// followed by
//   nt16 wshift
//   head_frag    the count of halves, then their bytes
//   use_first    1 (else 0 and nothing more), then
//   FirstParams  P Ci ks ntaps NT CW NKS rw_log2 hh hw inv_hw lds_bytes act post_affine Cds outS
//   first_w      the count of halves, then their bytes
unsigned long long tconv_digest(const ConvParams& c, int nt, int hpix, const PackDesc* packs, size_t npacks, const HostPlan* P) {
    Fnv d;
    d.is(nt, hpix, c.C[0], c.C[1], c.Cp[0], c.Cp[1], c.vec4[0], c.vec4[1], c.ngroups, c.H, c.W, c.Cout, c.Np, c.twm_log2, c.th_log2,
         c.nimg_m, c.imgs, c.hh, c.hw, c.imgplane, c.plane, c.ymin, c.xmin, c.tiles_y, c.tiles_x, c.nphase, c.o_mul);
    for (int ph = 0; ph < 4; ++ph)
        d.is(c.ph[ph].tap0[0], c.ph[ph].tap0[1], c.ph[ph].ntaps[0], c.ph[ph].ntaps[1], c.ph[ph].oy_off, c.ph[ph].ox_off);
    for (int t = 0; t < kMaxTaps; ++t) d.i(c.tapoff[t]);
    d.is(c.outH, c.outW, c.pool, c.act, c.ksplit, c.split_stride);
    d.i((long long)npacks);
    for (size_t k = 0; k < npacks; ++k) {
        const PackDesc& q = packs[k];
        d.is(q.ntaps, q.Cp, q.Np, q.C, q.N, q.d2, q.d3, q.transpose, q.c_off, q.npar, q.Cblk, q.bwd);
        for (int t = 0; t < 4 * kMaxPackTaps; ++t) d.i(q.mtap[t]);
    }
    d.i(P ? 1 : 0);
    if (P) digest_host_plan(d, *P);
    return d.v;
}

}  // namespace umx
