// yn_train.inc — the fp32 executor of the training step (SURVEY §8 row 20), included by yn_api.hip after yn_train_shared.inc.
//
// train.py:219-231 — `model(images, target)` in train mode (BatchNorm batch statistics), the four losses,
// `total_loss.backward()`, `optimizer.step()` — restated as an explicit forward tape + hand-written backward over the
// kernels of kernels_conv.hip / kernels_bwd.hip / kernels_train.hip.  Parameters, gradients and momentum live in three
// caller-owned FLAT float32 buffers (order = nn.Module.named_parameters() of the reference model), so the gradient
// exchange of data-parallel training is ONE all-reduce over `grads` between yn_train_step(do_update = 0) and yn_sgd_step.
//
// The network's wiring is train_tape (yn_train_tape.inc); this file is what one layer does in fp32: NHWC float32 tensors with their
// logical channel count, no buffer reuse within a step, weight packs allocated once in yn_train_bind and refilled from the flat
// parameter buffer at the start of every step.

namespace {

struct View { float* p; int ld, off, cs; };             // channel c of row m: p[m*ld + off + c*cs]
struct TT { float* v; float* g; long M; int C; };       // value + gradient, [M][C]

struct TRec {                                           // one conv (+BN +act) executed in train mode
    const Layer* l = nullptr;
    View x{};                                           // conv input (cs = 1)
    int B = 0, H = 0, W = 0;                            // input spatial extent
    long Mi = 0, Mo = 0;
    float* y = nullptr; int y_ld = 0;                   // conv output, pre-BN (the layer output itself when there is no BN)
    float *mean = nullptr, *invstd = nullptr;
    double* acc = nullptr;                              // [4][C] zeroed at step start: forward sums, backward sums
    const float* x_nchw = nullptr;                      // stem
};

// pack geometry of one layer: the same values yn_fold_bn derives
struct PackDims { int kind, kk, Kp, Npad; };
PackDims pack_dims(const Layer& l)
{
    if (l.kind == K_DW) return PackDims{1, 9, 9, l.cout};
    if (l.kind == K_STEM) return PackDims{2, 9, 27, l.cout};
    const int kk = l.kind == K_DENSE3 ? 9 : 1;
    return PackDims{0, kk, (l.cin * kk + 1) & ~1, (l.cout + 31) & ~31};
}

// ---- what one layer launches in fp32.  The step (Trainer, below) and the op-level entries (yn_train_ops.inc) both go through these, so
//      a kernel tested on its own runs behind the launch decisions the step makes for it. ----
struct BnPtrs { const float* gamma; const float* beta; float* rmean; float* rvar; float* dgamma; float* dbeta; };
// where a layer's parameter gradients go: dw is written (pointwise, dense, stem) or added to (depthwise: slot 0 of the gradient slots);
// the bias gradient of a BN-less conv is added into GRAD_SLOTS copies slot_stride floats apart; wpart is the per-slice scratch
struct GradPtrs { float* dw; float* dbias_slots; size_t slot_stride; float* wpart; size_t wpart_cap; };

// a layer's forward packs and (when it has them) backward packs from its raw weights; the packs' padding was zeroed when they were allocated
void fill_packs(const Layer& l, const TrainPack& pk, const float* w, const float* b, hipStream_t st)
{
    const PackDims d = pack_dims(l);
    FoldArgs a{};
    a.w = w; a.b = b; a.eps = 1e-5f; a.Cout = l.cout; a.Cin = l.cin;
    a.kind = d.kind; a.kk = d.kk; a.Kp = d.Kp; a.Npad = d.Npad;
    a.w_packed = pk.wp; a.b_packed = pk.bias;
    launch_fold_pack(a, st);
    if (pk.wp_bwd) {
        if (l.kind == K_DW) launch_pack_bwd(a.w, l.cout, 1, 1, 0, pk.wp_bwd, st);
        else launch_pack_bwd(a.w, l.cout, l.cin, l.kind == K_DENSE3 ? 2 : 0, pk.Npad_b, pk.wp_bwd, st);
    }
}
// per-layer packs (forward: raw weights; backward: transposed / flipped), zero-filled; sets the layer's pack geometry
int alloc_packs(yn_handle* h, Layer& l, TrainPack& pk)
{
    const PackDims d = pack_dims(l);
    const size_t fwd = (size_t)d.Kp * d.Npad, nbias = (size_t)((d.Npad + 31) & ~31);
    size_t bwd = l.kind == K_DW ? fwd : 0;
    if (l.kind == K_PW || l.kind == K_DENSE3) {
        pk.Kb = (l.cout * d.kk + 1) & ~1; pk.Npad_b = (l.cin + 31) & ~31; bwd = (size_t)pk.Kb * pk.Npad_b;
        if (l.kind == K_DENSE3) pk.Kb = l.cout;              // conv3x3 launcher takes Cin', not 9*Cin'
    }
    l.Kp = d.Kp; l.Npad = d.Npad;                              // the same values yn_fold_bn derives
    HIPCHK(h, pk.wp.reserve(fwd));
    HIPCHK(h, pk.bias.reserve(nbias));
    HIPCHK(h, hipMemsetAsync(pk.wp, 0, fwd * sizeof(float), h->stream));
    HIPCHK(h, hipMemsetAsync(pk.bias, 0, nbias * sizeof(float), h->stream));
    if (bwd) {
        HIPCHK(h, pk.wp_bwd.reserve(bwd));
        HIPCHK(h, hipMemsetAsync(pk.wp_bwd, 0, bwd * sizeof(float), h->stream));
    }
    return 0;
}
// y = conv(x) + bias into r.y (row stride r.y_ld; a pointwise conv also stores the zero-weight columns up to a padded r.y_ld)
void conv_forward(yn_handle* h, const TRec& r, const TrainPack& pk, hipStream_t st)
{
    const Layer& l = *r.l;
    const View& x = r.x;
    if (l.kind == K_PW) {
        GemmArgs a{};
        a.in = x.p; a.in_ld = x.ld; a.in_off = x.off; a.Wp = pk.wp; a.bias = pk.bias;
        a.out = r.y; a.out_ld = r.y_ld; a.M = (int)r.Mo; a.K = l.cin; a.N = r.y_ld <= l.Npad ? r.y_ld : l.cout; a.Npad = l.Npad; a.act = 0;
        a.cfg = tune_pw(h, a);      // per-shape tile choice, timed once (as in inference)
        launch_pw(a, st);
    } else if (l.kind == K_DW) {
        DwArgs a{};
        a.in = x.p; a.in_ld = x.ld; a.in_off = x.off; a.w = pk.wp; a.bias = pk.bias; a.out = r.y; a.out_ld = r.y_ld; a.out_off = 0;
        a.B = r.B; a.H = r.H; a.W = r.W; a.C = l.cout; a.stride = l.stride; a.act = 0;
        launch_dw(a, st);
    } else if (l.kind == K_DENSE3) {
        GemmArgs a{};
        a.in = x.p; a.in_ld = x.ld; a.in_off = x.off; a.resample = 0; a.H = r.H; a.W = r.W; a.Wp = pk.wp; a.bias = pk.bias;
        a.out = r.y; a.out_ld = r.y_ld; a.M = (int)r.Mo; a.K = l.cin; a.N = l.cout; a.Npad = l.Npad; a.act = 0; a.cfg = -1;
        launch_conv3x3(a, st);
    } else {
        launch_stem(r.x_nchw, r.B, r.H, r.W, pk.wp, pk.bias, l.cout, 0, r.y, st);
    }
}
// BatchNorm (batch statistics) + activation of r.y into `out`; optional concat+shuffle pass-through.  r.acc: [4][ACC_SLOTS][C] zeroed doubles
void bn_forward(const TRec& r, const BnPtrs& p, View out, View pass, hipStream_t st)
{
    const Layer& l = *r.l;
    launch_bn_stats(r.y, (int)r.Mo, l.cout, r.acc, st);
    BnApplyArgs a{};
    a.y = r.y; a.acc = r.acc; a.eps = 1e-5f; a.mean = r.mean; a.invstd = r.invstd; a.gamma = p.gamma; a.beta = p.beta;
    a.out = out.p; a.out_ld = out.ld; a.out_off = out.off; a.out_cs = out.cs;
    a.pass = pass.p; a.pass_ld = pass.ld; a.pass_off = pass.off; a.pass_dst_off = 0;
    a.rmean = p.rmean; a.rvar = p.rvar; a.momentum = 0.1f;
    a.M = (int)r.Mo; a.C = l.cout; a.act = l.act;
    launch_bn_apply(a, st);
}
// through activation + BatchNorm: dy over r.y IN PLACE, dgamma, dbeta
void bn_backward(const TRec& r, const BnPtrs& p, View dz, hipStream_t st)
{
    const Layer& l = *r.l;
    BnBwdArgs a{};
    a.dz = dz.p; a.dz_ld = dz.ld; a.dz_off = dz.off; a.dz_cs = dz.cs;
    a.y = r.y; a.mean = r.mean; a.invstd = r.invstd; a.gamma = p.gamma; a.beta = p.beta; a.dy = r.y; a.M = (int)r.Mo; a.C = l.cout; a.act = l.act;
    a.acc = r.acc + 2 * ACC_SLOTS * (size_t)l.cout; a.dgamma = p.dgamma; a.dbeta = p.dbeta;
    launch_bn_bwd(a, st);
}
// bias / weight gradients of one layer from dy
void param_grads(const TRec& r, const float* d, int d_ld, const GradPtrs& g, hipStream_t st)
{
    const Layer& l = *r.l;
    // a conv bias in front of a train-mode BatchNorm has an exactly zero gradient (the batch mean removes it): its
    // slice of the zeroed gradient buffer is left alone; torch computes round-off noise of ~1e-7 * |dy| there.
    if (g.dbias_slots) launch_col_sum_accumulate(d, d_ld, 0, (int)r.Mo, l.cout, g.dbias_slots, g.slot_stride, st);
    if (l.kind == K_PW || l.kind == K_DENSE3) {
        WgradArgs a{};
        a.dy = d; a.dy_ld = d_ld; a.x = r.x.p; a.x_ld = r.x.ld; a.x_off = r.x.off; a.H = r.H; a.W = r.W; a.Cin = l.cin;
        a.dense = l.kind == K_DENSE3; a.dw = g.dw; a.partial = g.wpart; a.partial_cap = g.wpart_cap; a.M = (int)r.Mo; a.N = l.cout; a.K = a.dense ? 9 * l.cin : l.cin;
        launch_wgrad(a, st);
    } else if (l.kind == K_DW) {
        launch_dw_wgrad(d, r.x.p, r.x.ld, r.x.off, r.B, r.H, r.W, l.cout, l.stride, g.dw, g.wpart, g.wpart_cap, st);
    } else {
        launch_stem_wgrad(d, r.x_nchw, r.B, r.H, r.W, l.cout, g.dw, g.wpart, g.wpart_cap, st);
    }
}
// gradient w.r.t. the conv input, written (or accumulated) into dx (cs = 1); tmp: [Mi][cin] scratch of the accumulate route
void input_grad(yn_handle* h, const TRec& r, const TrainPack& pk, const float* d, int d_ld, View dx, bool accumulate, float* tmp, hipStream_t st)
{
    const Layer& l = *r.l;
    if (l.kind == K_DW && l.stride == 2) {
        launch_dw_dgrad_s2(d, pk.wp, r.B, r.H, r.W, l.cout, dx.p, dx.ld, dx.off, accumulate ? 1 : 0, st);
        return;
    }
    View o = dx;
    if (accumulate) o = View{tmp, l.cin, 0, 1};
    if (l.kind == K_PW) {
        GemmArgs a{};
        a.in = d; a.in_ld = d_ld; a.in_off = 0; a.Wp = pk.wp_bwd; a.bias = h->zeros; a.out = o.p; a.out_ld = o.ld; a.out_off = o.off;
        a.M = (int)r.Mo; a.K = pk.Kb; a.N = l.cin; a.Npad = pk.Npad_b; a.act = 0; a.cfg = tune_pw(h, a);      // per-shape tile choice, timed once (as in inference)
        launch_pw(a, st);
    } else if (l.kind == K_DW) {
        DwArgs a{};
        a.in = d; a.in_ld = d_ld; a.in_off = 0; a.w = pk.wp_bwd; a.bias = h->zeros; a.out = o.p; a.out_ld = o.ld; a.out_off = o.off;
        a.B = r.B; a.H = r.H; a.W = r.W; a.C = l.cout; a.stride = 1; a.act = 0;
        launch_dw(a, st);
    } else if (l.kind == K_DENSE3) {
        GemmArgs a{};
        a.in = d; a.in_ld = d_ld; a.in_off = 0; a.resample = 0; a.H = r.H; a.W = r.W; a.Wp = pk.wp_bwd; a.bias = h->zeros;
        a.out = o.p; a.out_ld = o.ld; a.out_off = o.off; a.M = (int)r.Mo; a.K = l.cout; a.N = l.cin; a.Npad = pk.Npad_b; a.act = 0; a.cfg = -1;
        launch_conv3x3(a, st);
    }
    if (accumulate) launch_strided_copy(tmp, l.cin, 0, 1, dx.p, dx.ld, dx.off, 1, r.Mi, l.cin, 1, st);
}
// the even channels of a unit's output gradient g [M][C] (its pass-through half) as a copy of their own
void even_channels_to(const float* g, int C, long M, View dst, hipStream_t st) { launch_strided_copy(g, C, 0, 2, dst.p, dst.ld, dst.off, 1, M, C / 2, 0, st); }
int zeros_ready(yn_handle* h)
{
    if (!h->zeros) {
        HIPCHK(h, h->zeros.reserve(4096));
        HIPCHK(h, hipMemsetAsync(h->zeros, 0, 4096 * sizeof(float), h->stream));
    }
    return 0;
}

struct Trainer : StepBase<TRec> {
    using StepBase::StepBase;
    using Ten = TT;
    static constexpr int is_h16 = 0;
    struct Pending { const TRec* r; const float* d; int ld; };
    SideQueue<Pending> sq;
    float* tmp = nullptr;                               // the accumulate-scratch of back_input
    TT a0{}, a1{}; int32_t* pool_idx = nullptr; int r_stem = -1;      // the stem's tensors (stem_fwd / stem_bwd)

    float* take(size_t floats) { return (float*)ar.up(floats * sizeof(float)); }
    float* take_g(size_t floats) { return (float*)ar.down(floats * sizeof(float)); }
    TT mk(long M, int C) { return TT{take((size_t)M * C), take_g((size_t)M * C), M, C}; }
    TT mk_unit(long M, int bf) { return mk(M, 2 * bf); }                // a ShuffleV2 unit's output: x1 / branch2 interleaved
    TT mk_like(const TT& t, long M) { return mk(M, t.C); }
    static int head_ld(int ch) { return (ch + 3) & ~3; }                // raw-head rows padded to 16 bytes
    static View full(const TT& t, bool grad = false) { return View{grad ? t.g : t.v, t.C, 0, 1}; }
    static View plane(const TT& t, int which, bool grad = false) { return View{grad ? t.g : t.v, t.C, which ? t.C / 2 : 0, 1}; }   // a unit's input: x1 = [0, bf), x2 = [bf, 2bf)
    static View odd(const TT& t, bool grad = false) { return View{grad ? t.g : t.v, t.C, 1, 2}; }
    TT out_of(int ri, float* g) { return TT{recs[ri].y, g, recs[ri].Mo, recs[ri].y_ld}; }     // a BN-less conv's output as a tensor
    const TrainPack& pack(const Layer& l) { return h->tpacks[(size_t)(&l - &h->layers[0])]; }

    // workspace of the step, gradients at zero, weight packs from the current parameters (their padding was zeroed once in yn_train_bind)
    int begin()
    {
        const int HCp = head_ld(h->head_ch);
        // the largest dy / accumulate-scratch of any layer: the stem's 24 channels at S/2, or a padded head row at S/8
        const size_t stem = (size_t)B * (S / 2) * (S / 2) * 24, head = (size_t)B * (S / 8) * (S / 8) * HCp;
        tmp = take(stem > head ? stem : head);
        if (carve_scratch(h, ar, ACC_SLOTS, st, sc)) return 1;
        for (size_t i = 0; i < h->layers.size(); ++i) {
            const Layer& l = h->layers[i];
            fill_packs(l, h->tpacks[i], P(l.conv + ".weight"), l.has_bias ? P(l.conv + ".bias") : nullptr, st);
        }
        return 0;
    }

    // ---- forward pieces ----
    // a conv without BatchNorm (the heads' last one) writes the layer output itself, with the padded row stride head_ld (extra column = 0)
    int conv(const Layer& l, View x, int B_, int H, int W, const float* x_nchw = nullptr)
    {
        TRec r;
        r.l = &l; r.x = x; r.B = B_; r.H = H; r.W = W; r.x_nchw = x_nchw;
        const int Ho = (H - 1) / l.stride + 1, Wo = (W - 1) / l.stride + 1;
        r.Mi = (long)B_ * H * W; r.Mo = (long)B_ * Ho * Wo;
        r.y_ld = l.bn.empty() ? head_ld(l.cout) : l.cout;
        r.y = take((size_t)r.Mo * r.y_ld);
        conv_forward(h, r, pack(l), st);
        recs.push_back(r);
        return (int)recs.size() - 1;
    }
    // forward: the running statistics; backward: where dgamma / dbeta go
    BnPtrs bn_ptrs(const Layer& l, bool forward)
    {
        BnPtrs p{P(l.bn + ".weight"), P(l.bn + ".bias"), nullptr, nullptr, nullptr, nullptr};
        if (forward) {
            const Param* rm = find_param(h, l.bn + ".running_mean");
            const Param* rv = find_param(h, l.bn + ".running_var");
            p.rmean = rm ? (float*)rm->dev : nullptr; p.rvar = rv ? (float*)rv->dev : nullptr;
        } else { p.dgamma = G(l.bn + ".weight"); p.dbeta = G(l.bn + ".bias"); }
        return p;
    }
    // BatchNorm (batch statistics) + activation into `out`; optional concat+shuffle pass-through
    void bn_into(int ri, View out, View pass = View{nullptr, 0, 0, 1})
    {
        TRec& r = recs[ri];
        const Layer& l = *r.l;
        r.mean = take(l.cout); r.invstd = take(l.cout);
        r.acc = sc.take_stats(4 * ACC_SLOTS * (size_t)l.cout);
        if (!r.acc) { ar.oom = true; return; }
        bn_forward(r, bn_ptrs(l, true), out, pass, st);
    }
    void bn(int ri, const TT& out) { bn_into(ri, full(out)); }
    void bn_shuffle(int ri, View pass, const TT& unit) { bn_into(ri, odd(unit), pass); }      // unit[2c] = pass[c], unit[2c+1] = z[c]

    TT stem_fwd(const float* x_dev)
    {
        const int H1 = S / 2, H2 = S / 4;
        a0 = mk((long)B * H1 * H1, 24); a1 = mk((long)B * H2 * H2, 24);
        pool_idx = (int32_t*)take((size_t)a1.M * 24);
        r_stem = conv(L(h, "stem"), View{nullptr, 0, 0, 1}, B, S, S, x_dev);
        bn(r_stem, a0);
        launch_maxpool_idx(a0.v, B, H1, H1, 24, a1.v, pool_idx, st);
        return a1;
    }
    void stem_bwd()
    {
        launch_maxpool_bwd(a1.g, pool_idx, B, S / 2, S / 2, 24, a0.g, st);
        back(r_stem, full(a0, true), View{nullptr, 0, 0, 1}, false, false);
    }
    void resample(const float* a, const float* b, float* out, int W, int mode) { launch_resample(a, b, out, B, W, W, NECK, mode, st); }
    int forward_done() { return 0; }
    void loss(const TT hd[3], const float* target_dev, float* losses_dev)
    {
        GridInfo g = h->grid;
        g.head_ld = hd[0].C;
        const float* const heads[3] = {hd[0].v, hd[1].v, hd[2].v};
        float* const gheads[3] = {hd[0].g, hd[1].g, hd[2].g};
        launch_loss(nullptr, nullptr, nullptr, heads, gheads, target_dev, g, B, h->loss_partial, losses_dev, nullptr, nullptr, nullptr, st);
    }
    void combine() { launch_grad_combine(h->tG, sc.gslots, (long)h->tN, (size_t)h->tN, st); }

    // ---- backward pieces ----
    // gradient w.r.t. the conv output (through act + BN), parameter gradients of BN / bias / weights. Returns (dy, ld).
    const float* back_params(const TRec& r, View dz, int* dy_ld)
    {
        const Layer& l = *r.l;
        const float* d;
        if (!l.bn.empty()) {
            bn_backward(r, bn_ptrs(l, false), dz, st);                   // in place
            d = r.y; *dy_ld = l.cout;
        } else {
            d = dz.p + dz.off; *dy_ld = dz.ld;            // plain conv output (head): dz is dense, cs = 1
        }
        sq.add(st, Pending{&r, d, *dy_ld}, [this](const Pending& p) { params_on_side(*p.r, p.d, p.ld); });
        return d;
    }
    void flush_params() { sq.flush(st, [this](const Pending& p) { params_on_side(*p.r, p.d, p.ld); }); }
    // bias / weight gradients of one layer from dy, on the side stream when there is one
    void params_on_side(const TRec& r, const float* d, int d_ld)
    {
        const Layer& l = *r.l;
        hipStream_t st = sq.side ? sq.side : this->st;
        GradPtrs g{};
        g.dw = l.kind == K_DW ? GS(l.conv + ".weight") : G(l.conv + ".weight");
        g.dbias_slots = l.has_bias && l.bn.empty() ? GS(l.conv + ".bias") : nullptr; g.slot_stride = (size_t)h->tN;
        g.wpart = sc.wpart; g.wpart_cap = sc.wpart_cap;
        param_grads(r, d, d_ld, g, st);
    }
    // gradient w.r.t. the conv input, written (or accumulated) into dx (cs = 1)
    void back_input(const TRec& r, const float* d, int d_ld, View dx, bool accumulate) { input_grad(h, r, pack(*r.l), d, d_ld, dx, accumulate, tmp, st); }
    // whole layer backward: dz (gradient of the layer's output view) -> parameter grads + input gradient (`below` is the fp16 executor's hint)
    void back(int ri, View dz, View dx, bool accumulate, bool need_input = true, int /*below*/ = -1)
    {
        int ld = 0;
        const float* d = back_params(recs[ri], dz, &ld);
        if (need_input) back_input(recs[ri], d, ld, dx, accumulate);
    }
    // the even channels of a unit's output gradient (its pass-through half) as a copy of their own ...
    void even_to(const TT& unit, View dst) { even_channels_to(unit.g, unit.C, unit.M, dst, st); }
    // ... issued before pw2's backward (from the odd channels) in a stride-1 unit, left to the tape (false) in a stride-2 unit
    void back_unit_s1(int ri, const TT& unit, View dx, View even_dst, int below) { even_to(unit, even_dst); back(ri, odd(unit, true), dx, false, true, below); }
    bool back_unit_s2(int ri, const TT& unit, View dx, View, int below) { back(ri, odd(unit, true), dx, false, true, below); return false; }
};

}  // namespace
