// The stream schedule of the v2 training step on the host: step_plan returns, as plain data, every step enqueue_step (umx_train.hip)
// enqueues -- in host order, with the stream it goes to, the events that stream waits on before it and records after it, and the
// buffers it reads and writes.  No HIP call, no trainer, no getenv: the schedule can be read, diffed and checked for hazards without
// a device (umx_test_step_plan, tests/test_step_plan_cpu.py, tools/tstep_plan_main.hip).
//
// The shape of the step: the main stream runs the dependent chain (forward pass, loss, then per site the gradient w.r.t. the conv
// output and the input-gradient convolutions).  The weight gradients hang off that chain: they run on two side streams against kSlots
// dz / gS slots the sites take in turn (slot & 1 picks the side stream, which owns the slice workspace ws / ws2).  On the
// split-precision route the skip connections' input gradients, needed only on the way back down the U, run on the aux stream.  Before
// its first weight gradient side stream 0 packs the backward pass's operands and sums the regularisation loss under the forward pass.
#include "umx_internal.h"

namespace umx {
namespace {

struct Builder {
    StepPlan p;
    // a step on `stream`; its reads and writes follow by rd / wr, its events by wait / rec
    TStep& add(int op, int site, int stream) {
        TStep s = {};
        s.op = (unsigned char)op; s.site = (unsigned char)site; s.stream = (unsigned char)stream;
        s.r0 = s.w0 = (unsigned short)p.bufs.size();
        p.steps.push_back(s);
        return p.steps.back();
    }
    void rd(std::initializer_list<int> ids) {
        TStep& s = p.steps.back();
        for (int id : ids) p.bufs.push_back((unsigned short)id);
        s.nr = (unsigned char)(s.nr + ids.size());
        s.w0 = (unsigned short)p.bufs.size();
    }
    void wr(std::initializer_list<int> ids) {   // (after the step's reads)
        TStep& s = p.steps.back();
        for (int id : ids) p.bufs.push_back((unsigned short)id);
        s.nw = (unsigned char)(s.nw + ids.size());
    }
    void wait(int ev) { TStep& s = p.steps.back(); s.wait[s.nwait++] = (unsigned char)ev; }
    void rec(int ev) { TStep& s = p.steps.back(); s.rec[s.nrec++] = (unsigned char)ev; }
};

}  // namespace

StepPlan step_plan(const StepEnv& env) {
    const int L = env.L, top = site_top(L);
    Builder b;
    b.p.L = L;
    b.p.nevents = TE_SKIP + L;
    const bool use_aux = env.hconv;   // the skip convolutions that took the split-precision route leave the main stream

    // ---- forward: side stream 0 packs the backward operands and sums the regularisation loss under the main stream's forward pass
    b.add(T_BEGIN, 0, TS_MAIN); b.wr({tbuf(TB_LOSS0), tbuf(TB_LOSS1)}); b.rec(TE_BEGIN);
    b.add(T_PACK0, 0, TS_MAIN); b.wr({tbuf(TB_FPACK)});
    b.add(T_PACK1, 0, TS_SIDE0); b.wr({tbuf(TB_BPACK)}); b.wait(TE_BEGIN);
    if (env.reg) { b.add(T_REG, 0, TS_SIDE0); b.wr({tbuf(TB_PART2), tbuf(TB_LOSS1)}); }
    b.rec(TE_PACKED);
    b.add(T_FWD, 0, TS_MAIN);   // forward_pass as one step: the eval pass shares it
    b.rd({tbuf(TB_DS, 0), tbuf(TB_FPACK)});
    for (int i = 1; i <= L; ++i) b.wr({tbuf(TB_DS, i)});
    b.wr({tbuf(TB_ACTB)});
    for (int i = 0; i < L; ++i) b.wr({tbuf(TB_US, i), tbuf(TB_CV, i)});
    for (int s = 0; s <= top; ++s) b.wr({tbuf(TB_Z, s), tbuf(TB_STAT, s)});
    b.wr({tbuf(TB_PART), tbuf(TB_SPLIT)});
    b.add(T_LOSS, 0, TS_MAIN); b.rd({tbuf(TB_Z, top), tbuf(TB_STAT, top)}); b.wr({tbuf(TB_DT), tbuf(TB_PART), tbuf(TB_LOSS0)});
    b.add(T_MARK, 0, TS_MAIN); b.wait(TE_PACKED);   // the backward pass's operands are in place
    b.add(T_HEAD, top, TS_MAIN);   // softmax/CE gradient -> BN -> 1x1 conv
    b.rd({tbuf(TB_DT), tbuf(TB_Z, top), tbuf(TB_STAT, top), tbuf(TB_CV, 0)});
    b.wr({tbuf(TB_DT), tbuf(TB_M12, top), tbuf(TB_PART), tbuf(TB_DA), tbuf(TB_G_BN, top), tbuf(TB_G_LT)});

    // ---- backward: the 2 L + 1 sites take the slots in turn
    int slot = 0;
    bool used[kSlots] = {}, aux_used[kSlots] = {};
    // the gradient w.r.t. site's conv output from dy0 (+ dskip), into the current slot: main waits for the slot's previous readers on
    // the side and aux streams, and side stream slot & 1 for main
    auto dz = [&](int site, int dy0, int dskip, int skip_ev) {
        b.add(T_DZ, site, TS_MAIN);
        b.rd({dy0, tbuf(TB_Z, site), tbuf(TB_STAT, site)});
        if (dskip >= 0) b.rd({dskip});
        b.wr({tbuf(TB_DZ, slot), tbuf(TB_M12, site), tbuf(TB_PART), tbuf(TB_G_BN, site)});
        if (skip_ev >= 0) b.wait(skip_ev);
        if (used[slot]) b.wait(TE_SIDE + slot);
        if (aux_used[slot]) { b.wait(TE_AUX + slot); aux_used[slot] = false; }
        b.rec(TE_DZ + slot);
    };
    // a weight gradient of the site on the slot's side stream (with that stream's slice workspace), into gradient segment g; wait_ev:
    // what main records once the slot is written, for the first reader of it
    auto wgrad = [&](int op, int site, int X, int G, int g, int wait_ev) {
        b.add(op, site, TS_SIDE0 + (slot & 1));
        b.rd({X, G});
        b.wr({g, tbuf(slot & 1 ? TB_WS2 : TB_WS)});
        if (wait_ev >= 0) b.wait(wait_ev);
    };
    auto conv = [&](int op, int site, int stream, int src, int dst) {
        b.add(op, site, stream);
        b.rd({src, tbuf(TB_BPACK)});
        b.wr({dst, tbuf(stream == TS_MAIN ? TB_SPLIT : stream == TS_AUX ? TB_SPLIT3 : TB_SPLIT2)});
    };
    auto next_slot = [&]() { b.rec(TE_SIDE + slot); used[slot] = true; slot = (slot + 1) % kSlots; };   // (on the slot's last weight gradient)
    for (int idx = 0; idx < L; ++idx) {   // up layers, output side first
        const int s = site_up(idx), DZ = tbuf(TB_DZ, slot), GS = tbuf(TB_GS, slot);
        dz(s, tbuf(TB_DA), -1, -1);
        wgrad(T_WG_U0, s, tbuf(TB_DS, idx), DZ, tbuf(TB_G_W2, idx), TE_DZ + slot);
        wgrad(T_WG_U1, s, tbuf(TB_US, idx), DZ, tbuf(TB_G_W2, idx), -1);
        conv(T_CV_US, s, TS_MAIN, DZ, tbuf(TB_DB));
        if (idx >= 1 && use_aux && env.skip_split[idx]) {
            conv(T_CV_SKIP, s, TS_AUX, DZ, tbuf(TB_DSKIP, idx));
            b.wait(TE_DZ + slot); b.rec(TE_AUX + slot); b.rec(TE_SKIP + idx);
            aux_used[slot] = true;
        } else if (idx >= 1) {
            conv(T_CV_SKIP, s, TS_MAIN, DZ, tbuf(TB_DSKIP, idx));
        }
        b.add(T_S2D, s, TS_MAIN); b.rd({tbuf(TB_DB), tbuf(TB_US, idx)}); b.wr({GS});
        // (in front of the event: the transposed convolution's weight gradient stages from these planes too)
        if (env.hconv && (env.T_split[idx] || env.wg_planes)) { b.add(T_GSP, s, TS_MAIN); b.rd({GS}); b.wr({GS}); }
        b.rec(TE_GS + slot);
        // (the transposed convolution's filter: X is gS, G the layer's input)
        wgrad(T_WG_T, s, GS, idx == L - 1 ? tbuf(TB_ACTB) : tbuf(TB_CV, idx + 1), tbuf(TB_G_WT, idx), TE_GS + slot);
        const int cur = slot;
        next_slot();
        conv(T_CV_T, s, TS_MAIN, tbuf(TB_GS, cur), tbuf(TB_DA));
    }
    {   // bottom layer
        const int s = site_bottom(L), DZ = tbuf(TB_DZ, slot);
        dz(s, tbuf(TB_DA), -1, -1);
        wgrad(T_WG_B, s, tbuf(TB_DS, L), DZ, tbuf(TB_G_LB), TE_DZ + slot);
        next_slot();
        conv(T_CV_B, s, TS_MAIN, DZ, tbuf(TB_DB));
    }
    for (int i = L - 1; i >= 0; --i) {   // down layers
        const int s = site_down(L, i), DZ = tbuf(TB_DZ, slot);
        const bool skip = i + 1 <= L - 1;
        dz(s, tbuf(TB_DB), skip ? tbuf(TB_DSKIP, i + 1) : -1, skip && use_aux && env.skip_split[i + 1] ? TE_SKIP + i + 1 : -1);
        wgrad(T_WG_D, s, tbuf(TB_DS, i), DZ, tbuf(TB_G_WD, i), TE_DZ + slot);
        next_slot();
        if (i >= 1) conv(T_CV_D, s, TS_MAIN, DZ, tbuf(TB_DB));
    }
    // ---- join: the optimiser (and the caller) see every gradient
    for (int k = 0; k < 2; ++k) { b.add(T_JOIN, 0, TS_SIDE0 + k); b.rec(TE_JOIN + k); }
    b.add(T_OPT, 0, TS_MAIN);
    b.rd({tbuf(TB_G_LT), tbuf(TB_G_LB)});
    for (int i = 0; i < L; ++i) b.rd({tbuf(TB_G_W2, i), tbuf(TB_G_WT, i), tbuf(TB_G_WD, i)});
    for (int s = 0; s <= top; ++s) b.rd({tbuf(TB_G_BN, s)});
    b.wait(TE_JOIN); b.wait(TE_JOIN + 1);
    return b.p;
}

namespace {

const char* const kOpNames[T_NOPS] = {"begin", "pack0", "pack1", "reg", "forward", "loss", "mark", "head", "dz", "wgrad.u0", "wgrad.u1",
                                      "wgrad.T", "wgrad.b", "wgrad.d", "conv.us", "conv.skip", "conv.T", "conv.b", "conv.d", "s2d",
                                      "gsplanes", "join", "opt"};
const char* const kStreamNames[kStepStreams] = {"main", "side0", "side1", "aux"};
const char* const kBufNames[TB_NKINDS] = {"ds", "us", "cv", "actb", "z.", "stat.", "m12.", "DA", "DB", "dt", "dskip", "dz", "gs", "part", "part2",
                                          "ws", "ws2", "split", "split2", "split3", "fpack", "bpack", "loss0", "loss1",
                                          "g.lt", "g.w2.", "g.wt.", "g.lb", "g.wd.", "g.bn."};

std::string site_name(int s, int L) {
    if (s == site_top(L)) return "t";
    if (s == site_bottom(L)) return "b";
    return s < L ? "u" + std::to_string(s) : "d" + std::to_string(2 * L - s);
}

std::string buf_name(int id, int L) {
    const int kind = id / 32, index = id % 32;
    const std::string nm = kBufNames[kind];
    if (kind == TB_Z || kind == TB_STAT || kind == TB_M12 || kind == TB_G_BN) return nm + site_name(index, L);
    const bool indexed = kind == TB_DS || kind == TB_US || kind == TB_CV || kind == TB_DSKIP || kind == TB_DZ || kind == TB_GS ||
                         kind == TB_G_W2 || kind == TB_G_WT || kind == TB_G_WD;
    return indexed ? nm + std::to_string(index) : nm;
}

std::string event_name(int e) {
    if (e == TE_BEGIN) return "begin";
    if (e == TE_PACKED) return "packed";
    const char* const roles[] = {"join", "dz", "gs", "side", "aux", "skip"};
    const int base[] = {TE_JOIN, TE_DZ, TE_GS, TE_SIDE, TE_AUX, TE_SKIP};
    int r = 5;
    while (e < base[r]) --r;
    return roles[r] + std::to_string(e - base[r]);
}

}  // namespace

std::string step_describe(const StepPlan& p) {
    std::string out;
    for (const TStep& s : p.steps) {
        const bool sited = s.op >= T_HEAD && s.op <= T_GSP;
        out += std::string(kOpNames[s.op]) + " " + (sited ? site_name(s.site, p.L) : "-") + " " + kStreamNames[s.stream] + "; wait";
        for (int k = 0; k < s.nwait; ++k) out += " " + event_name(s.wait[k]);
        out += s.nwait ? "; record" : " -; record";
        for (int k = 0; k < s.nrec; ++k) out += " " + event_name(s.rec[k]);
        out += s.nrec ? "; r" : " -; r";
        for (int k = 0; k < s.nr; ++k) out += " " + buf_name(p.rd(s, k), p.L);
        out += s.nr ? "; w" : " -; w";
        for (int k = 0; k < s.nw; ++k) out += " " + buf_name(p.wr(s, k), p.L);
        out += s.nw ? "\n" : " -\n";
    }
    return out;
}

}  // namespace umx
