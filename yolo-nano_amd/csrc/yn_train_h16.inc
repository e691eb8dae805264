// yn_train_h16.inc — the fp16 executor of the training step (BASELINE configs[2]: "SGD training step fp16"), included by yn_api.hip
// after yn_train.inc.  Same tape (train_tape, yn_train_tape.inc; train.py:219-231; models/yolo_nano.py:282-358;
// backbone/shufflenetv2.py:69-78), different arithmetic: fp16 storage of activations / activation gradients in the
// channel-padded layout of kernels_h16.hip, f16 MFMA with fp32 accumulation for every GEMM-shaped conv, fp32 master weights
// (the caller's flat buffers, unchanged), fp32 BatchNorm statistics / parameter gradients, dynamic loss scale on the device.
// yn_train_step dispatches here when yn_train_precision(h, YN_F16) was called.

namespace {

inline int r8(int c) { return (c + 7) & ~7; }
inline int r32(int c) { return (c + 31) & ~31; }

struct HTen { h16* v; h16* g; long M; int C, Cp, half, gap; };                 // value + gradient, channel map (kernels_h16.hip)
struct HV { h16* p; int ld, off, C, Cp, half, gap; };                          // view: C logical channels in Cp physical ones starting at off

struct HRec {
    const Layer* l = nullptr;
    HV x{};
    int B = 0, H = 0, W = 0;
    long Mi = 0, Mo = 0;
    h16* y = nullptr; int oC = 0, Np = 0, ohalf = 0, ogap = 0;               // conv output [Mo][Np] and its channel map
    float *mean = nullptr, *invstd = nullptr;
    double* acc = nullptr;
    bool stats_done = false, sums_done = false;                               // the producing conv / the consuming conv's input gradient already took the column sums (HColStat)
    const float* x_nchw = nullptr;
};

struct HTrainer : StepBase<HRec> {
    using StepBase::StepBase;
    using Ten = HTen;
    static constexpr int is_h16 = 1;
    struct Pending { const HRec* r; const h16* d; };
    SideQueue<Pending> sq;
    HTen a0{}, a1{}; uint8_t* pool_idx = nullptr; int r_stem = -1;              // the stem's tensors (stem_fwd / stem_bwd)

    h16* take(size_t halves) { return (h16*)ar.up(halves * sizeof(h16)); }
    h16* take_g(size_t halves) { return (h16*)ar.down(halves * sizeof(h16)); }
    HTen mk(long M, int C) { return HTen{take((size_t)M * r8(C)), take_g((size_t)M * r8(C)), M, C, r8(C), C, 0}; }
    HTen mk_unit(long M, int bf) { const int bfp = r8(bf); return HTen{take((size_t)M * 2 * bfp), take_g((size_t)M * 2 * bfp), M, 2 * bf, 2 * bfp, bf, bfp - bf}; }
    HTen mk_like(const HTen& t, long M) { return HTen{take((size_t)M * t.Cp), take_g((size_t)M * t.Cp), M, t.C, t.Cp, t.half, t.gap}; }     // channel-wise: t's map
    static int head_ld(int ch) { return r8(ch); }
    static HV full(const HTen& t, bool grad = false) { return HV{grad ? t.g : t.v, t.Cp, 0, t.C, t.Cp, t.half, t.gap}; }
    // one plane of a gapped unit tensor: x1 = logical [0, bf), x2 = logical [bf, 2bf)
    static HV plane(const HTen& t, int which, bool grad = false) { return HV{grad ? t.g : t.v, t.Cp, which ? t.half + t.gap : 0, t.half, t.half + t.gap, t.half, 0}; }
    HTen out_of(int ri, h16* g) { const HRec& r = recs[ri]; return HTen{r.y, g, r.Mo, r.oC, r.Np, r.ohalf, r.ogap}; }     // a BN-less conv's output as a tensor
    HPack& pack(const Layer& l) { return h->hpacks[(size_t)(&l - &h->layers[0])]; }

    // streams of the step (created by train_step_h16), its scratch, gradients at zero, all weight packs from the current master weights
    int begin()
    {
        if (h->multi_stream && !h->profiling && h->train_side && h->train_events.size() >= (size_t)NEV + 1) sq.attach(h, h->train_side);
        if (sq.side && h->train_fork[0] && h->train_fork[1] && h->train_events.size() >= (size_t)NEV + 9) {
            if (h->head_fork_now) { sq.fk[0] = h->train_fork[0]; sq.fk[1] = h->train_fork[1]; }
            for (int i = 0; i < 8; ++i) sq.fev[i] = h->train_events[NEV + 1 + i];
        }
        if (carve_scratch(h, ar, HACC_SLOTS, st, sc)) return 1;
        if (h->hpack_table) launch_hpack_all(h->hpack_table, (int)h->hpack_table.cap(), st);
        return 0;
    }

    // (re)build the layer's packs from the fp32 master weights for the channel map of its input view
    int prepare(const Layer& l, const HV& x)
    {
        if (h->hpack_table) return 0;                        // steady state: every pack was rebuilt by ONE launch at the start of the step
        HPack& pk = pack(l);
        const float* w = P(l.conv + ".weight");
        const float* b = l.has_bias ? P(l.conv + ".bias") : nullptr;
        if (l.kind == K_DW) {
            if (!pk.dwf) {
                if (pk.dwb.reserve((size_t)9 * x.Cp) || pk.bias.reserve((size_t)x.Cp) || pk.dwf.reserve((size_t)9 * x.Cp)) return 1;     // dwf last: it marks the set as made
                (void)hipMemsetAsync(pk.dwf, 0, (size_t)9 * x.Cp * sizeof(float), st);
                (void)hipMemsetAsync(pk.dwb, 0, (size_t)9 * x.Cp * sizeof(float), st);
                (void)hipMemsetAsync(pk.bias, 0, (size_t)x.Cp * sizeof(float), st);
                pk.Kp = x.Cp;
            }
            launch_hpack_dw(w, b, l.cout, x.half, x.gap, x.Cp, 0, pk.dwf, pk.bias, st);
            if (l.stride == 1) launch_hpack_dw(w, nullptr, l.cout, x.half, x.gap, x.Cp, 1, pk.dwb, nullptr, st);
            h->hpack_jobs.push_back(HPackDesc{w, b, 1, l.cout, l.cin, 9, x.half, x.gap, x.Cp, 0, 0, 0, nullptr, nullptr, pk.bias, pk.dwf, l.stride == 1 ? pk.dwb : nullptr});
        } else if (l.kind == K_STEM) {
            if (pk.dwf.reserve((size_t)27 * 24)) return 1;
            launch_hpack_stem(w, pk.dwf, st);
            h->hpack_jobs.push_back(HPackDesc{w, nullptr, 2, 24, 3, 9, 3, 0, 0, 0, 0, 0, nullptr, nullptr, nullptr, pk.dwf, nullptr});
        } else {
            const int taps = l.kind == K_DENSE3 ? 9 : 1;
            if (!pk.wf) {
                pk.Kp = x.Cp; pk.Npad = r32(l.cout); pk.Kpb = r8(l.cout); pk.Npadb = r32(x.Cp);
                const size_t nf = (size_t)taps * pk.Kp * pk.Npad, nb = (size_t)taps * pk.Kpb * pk.Npadb;
                if (pk.wb.reserve(nb) || pk.bias.reserve((size_t)pk.Npad) || pk.wf.reserve(nf)) return 1;     // wf last: it marks the set as made
                (void)hipMemsetAsync(pk.wf, 0, nf * sizeof(h16), st);
                (void)hipMemsetAsync(pk.wb, 0, nb * sizeof(h16), st);
                (void)hipMemsetAsync(pk.bias, 0, (size_t)pk.Npad * sizeof(float), st);
            }
            launch_hpack_gemm(w, l.cout, l.cin, taps, x.half, x.gap, pk.Kp, pk.Npad, 0, pk.wf, st);
            launch_hpack_gemm(w, l.cout, l.cin, taps, x.half, x.gap, pk.Kpb, pk.Npadb, 1, pk.wb, st);
            if (b) (void)hipMemcpyAsync(pk.bias, b, (size_t)l.cout * sizeof(float), hipMemcpyDeviceToDevice, st);
            h->hpack_jobs.push_back(HPackDesc{w, b, 0, l.cout, l.cin, taps, x.half, x.gap, pk.Kp, pk.Npad, pk.Kpb, pk.Npadb, pk.wf, pk.wb, pk.bias, nullptr, nullptr});
        }
        return 0;
    }

    // ---- forward pieces ----
    int conv(const Layer& l, HV x, int B_, int H, int W, const float* x_nchw = nullptr)
    {
        HRec r;
        r.l = &l; r.x = x; r.B = B_; r.H = H; r.W = W; r.x_nchw = x_nchw;
        const int Ho = (H - 1) / l.stride + 1, Wo = (W - 1) / l.stride + 1;
        r.Mi = (long)B_ * H * W; r.Mo = (long)B_ * Ho * Wo;
        if (l.kind == K_DW) { r.oC = x.C; r.Np = x.Cp; r.ohalf = x.half; r.ogap = x.gap; }
        else { r.oC = l.cout; r.Np = r8(l.cout); r.ohalf = l.cout; r.ogap = 0; }
        r.y = take((size_t)r.Mo * r.Np);
        if (!l.bn.empty()) {
            r.mean = (float*)ar.up((size_t)l.cout * sizeof(float)); r.invstd = (float*)ar.up((size_t)l.cout * sizeof(float));
            r.acc = sc.take_stats(4 * HACC_SLOTS * (size_t)l.cout);
            if (!r.acc) { ar.oom = true; recs.push_back(r); return (int)recs.size() - 1; }
        }
        if (prepare(l, x)) { ar.oom = true; recs.push_back(r); return (int)recs.size() - 1; }
        const HPack& pk = pack(l);
        if (l.kind == K_PW || l.kind == K_DENSE3) {
            HGemmArgs a{};
            a.in = x.p; a.in_ld = x.ld; a.in_off = x.off; a.H = H; a.W = W; a.taps = l.kind == K_DENSE3 ? 9 : 1;
            a.Wp = pk.wf; a.bias = pk.bias; a.out = r.y; a.out_ld = r.Np; a.out_off = 0;
            a.M = (int)r.Mo; a.Kp = pk.Kp; a.Np = r.Np; a.Npad = pk.Npad; a.accumulate = 0;
            if (r.acc && sw.fuse_stats) { a.st.acc = r.acc; a.st.C = r.oC; a.st.half = r.ohalf; a.st.gap = r.ogap; r.stats_done = true; }      // BatchNorm statistics in the epilogue
            launch_hgemm(a, st);
        } else if (l.kind == K_DW) {
            HDwArgs a{};
            a.in = x.p; a.in_ld = x.ld; a.in_off = x.off; a.w = pk.dwf; a.bias = pk.bias; a.out = r.y; a.out_ld = r.Np; a.out_off = 0;
            a.B = B_; a.H = H; a.W = W; a.Cp = x.Cp; a.stride = l.stride; a.accumulate = 0;
            if (r.acc && sw.fuse_stats && l.stride == 1 && x.Cp <= 256) { a.st.acc = r.acc; a.st.C = r.oC; a.st.half = r.ohalf; a.st.gap = r.ogap; r.stats_done = true; }   // statistics in the run kernel's epilogue
            launch_hdw(a, st);
        } else {
            launch_hstem(x_nchw, B_, H, W, pk.dwf, nullptr, r.y, st);
        }
        recs.push_back(r);
        return (int)recs.size() - 1;
    }
    // the statistics (taken here when the conv's epilogue did not) and the BatchNorm + activation arguments of layer ri
    HBnApplyArgs bn_args(int ri)
    {
        HRec& r = recs[ri];
        const Layer& l = *r.l;
        const Param* rm = find_param(h, l.bn + ".running_mean");
        const Param* rv = find_param(h, l.bn + ".running_var");
        HRedArgs q{};
        q.y = r.y; q.y_ld = r.Np; q.y_off = 0; q.M = (int)r.Mo; q.C = r.oC; q.Cp = r.Np; q.half = r.ohalf; q.gap = r.ogap; q.acc = r.acc;
        if (!r.stats_done) launch_hcol_reduce(q, 0, st);
        HBnApplyArgs a{};
        a.y = r.y; a.y_ld = r.Np; a.acc = r.acc; a.eps = 1e-5f; a.M = (int)r.Mo; a.C = r.oC; a.Cp = r.Np; a.half = r.ohalf; a.gap = r.ogap; a.act = l.act;
        a.mean = r.mean; a.invstd = r.invstd; a.gamma = P(l.bn + ".weight"); a.beta = P(l.bn + ".bias");
        a.rmean = rm ? (float*)rm->dev : nullptr; a.rvar = rv ? (float*)rv->dev : nullptr; a.momentum = 0.1f;
        return a;
    }
    // BatchNorm (batch statistics) + activation, dense into `out` (same channel map as the conv output) ...
    void bn(int ri, const HTen& out)
    {
        if (!recs[ri].acc) { ar.oom = true; return; }
        HBnApplyArgs a = bn_args(ri);
        a.out = out.v; a.out_ld = out.Cp; a.out_off = 0;
        launch_hbn_apply(a, st);
    }
    // ... or as the concat+shuffle of a ShuffleV2 unit into the gapped tensor `unit`: unit[2c] = pass[c], unit[2c+1] = z[c]
    void bn_shuffle(int ri, HV pass, const HTen& unit)
    {
        if (!recs[ri].acc) { ar.oom = true; return; }
        HBnApplyArgs a = bn_args(ri);
        a.out = unit.v; a.out_ld = unit.Cp; a.out_off = 0; a.pass = pass.p; a.pass_ld = pass.ld; a.pass_off = pass.off; a.out_half = unit.half; a.out_gap = unit.gap;
        launch_hbn_apply(a, st);
    }

    // The stem's BatchNorm + activation + 3x3 / 2 max pool as one kernel (-> a1, arg-max positions), its backward without the full-resolution
    // gradient (kernels_h16.hip, hstem_apply_pool_kernel / hstem_bwd_kernel); sw.stem_fuse = 0: the separate launches, for the tests
    HTen stem_fwd(const float* x_dev)
    {
        const int H1 = S / 2, H2 = S / 4;
        a1 = mk((long)B * H2 * H2, 24);
        if (!sw.stem_fuse) a0 = mk((long)B * H1 * H1, 24);
        pool_idx = (uint8_t*)ar.up((size_t)a1.M * 24);
        r_stem = conv(L(h, "stem"), HV{nullptr, 0, 0, 3, 8, 3, 0}, B, S, S, x_dev);
        if (!sw.stem_fuse) {
            bn(r_stem, a0);
            launch_hmaxpool_idx(a0.v, B, H1, H1, 24, a1.v, pool_idx, st);
        } else if (!recs[r_stem].acc) ar.oom = true;
        else launch_hstem_apply_pool(bn_args(r_stem), B, H1, H1, a1.v, pool_idx, st);
        return a1;
    }
    // the way back: the pool's gather feeds the BatchNorm-backward sums and the in-place dy directly; then the stem conv's weight gradient
    void stem_bwd()
    {
        const int H1 = S / 2;
        if (!sw.stem_fuse) {
            launch_hmaxpool_bwd(a1.g, pool_idx, B, H1, H1, 24, a0.g, st);
            back(r_stem, full(a0, true), HV{}, false, false);
            return;
        }
        const HRec& r = recs[r_stem];
        const Layer& l = *r.l;
        HRedArgs q{};
        q.y = r.y; q.y_ld = r.Np; q.y_off = 0; q.M = (int)r.Mo; q.C = r.oC; q.Cp = r.Np; q.half = r.ohalf; q.gap = r.ogap;
        q.mean = r.mean; q.invstd = r.invstd; q.gamma = P(l.bn + ".weight"); q.beta = P(l.bn + ".bias"); q.act = l.act;
        q.acc = r.acc + 2 * HACC_SLOTS * (size_t)l.cout;
        launch_hstem_bwd(q, a1.g, pool_idx, B, H1, H1, r.y, G(l.bn + ".weight"), G(l.bn + ".bias"), st);
        queue_params(r, r.y);
    }
    void resample(const h16* a, const h16* b, h16* out, int W, int mode) { launch_hresample(a, b, out, B, W, W, NECK, mode, st); }
    // the first step packed layer by layer and recorded the jobs: upload the table
    int forward_done()
    {
        if (h->hpack_table || h->hpack_jobs.empty()) return 0;
        HIPCHK(h, h->hpack_table.reserve(h->hpack_jobs.size()));
        HIPCHK(h, hipMemcpyAsync(h->hpack_table, h->hpack_jobs.data(), h->hpack_jobs.size() * sizeof(HPackDesc), hipMemcpyHostToDevice, st));
        HIPCHK(h, hipStreamSynchronize(st));
        return 0;
    }
    // (+ scaled gradient w.r.t. the raw heads)
    void loss(const HTen hd[3], const float* target_dev, float* losses_dev)
    {
        GridInfo g = h->grid;
        g.head_ld = hd[0].Cp;
        const h16* const heads[3] = {hd[0].v, hd[1].v, hd[2].v};
        h16* const gheads[3] = {hd[0].g, hd[1].g, hd[2].g};
        launch_loss_h16(heads, gheads, target_dev, g, B, h->loss_partial, losses_dev, h->scale_state, st);
    }
    void combine() { launch_hgrad_finish(h->tG, sc.gslots, (long)h->tN, (size_t)h->tN, h->scale_state, st); }   // combine the slots, remove the loss scale, adapt it

    // ---- backward pieces ----
    // dz: gradient of the layer's BN+act output — a dense view with the conv output's map, or (odd_of != null) the odd logical
    // channels of the gapped unit gradient.  Returns dy (dense [Mo][Np]).
    const h16* back_params(const HRec& r, HV dz, const HTen* odd_of, HV* even)
    {
        const Layer& l = *r.l;
        const h16* d;
        if (!l.bn.empty()) {
            h16* dy = r.y;                                        // in place
            HRedArgs q{};
            q.y = r.y; q.y_ld = r.Np; q.y_off = 0; q.M = (int)r.Mo; q.C = r.oC; q.Cp = r.Np; q.half = r.ohalf; q.gap = r.ogap;
            if (odd_of) { q.dz = odd_of->g; q.dz_ld = odd_of->Cp; q.dz_off = 0; q.dz_odd = 1; q.dz_half = odd_of->half; q.dz_gap = odd_of->gap; }
            else { q.dz = dz.p; q.dz_ld = dz.ld; q.dz_off = dz.off; q.dz_odd = 0; }
            q.mean = r.mean; q.invstd = r.invstd; q.gamma = P(l.bn + ".weight"); q.beta = P(l.bn + ".bias"); q.act = l.act;
            q.acc = r.acc + 2 * HACC_SLOTS * (size_t)l.cout;
            if (even) { q.even = even->p; q.even_ld = even->ld; }                                    // the pass-through half leaves with the same loads
            launch_hbn_bwd(q, dy, G(l.bn + ".weight"), G(l.bn + ".bias"), st, r.sums_done);
            d = dy;
        } else {
            d = dz.p + dz.off;                                     // plain conv output (head): dense [Mo][Np]
        }
        queue_params(r, d);
        return d;
    }
    void queue_params(const HRec& r, const h16* d) { sq.add(st, Pending{&r, d}, [this](const Pending& p) { params_on_side(*p.r, p.d); }); }
    // (queued weight gradients belong to the stream they were queued on: the tape flushes before it moves to a tower's stream and back)
    void flush_params() { sq.flush(st, [this](const Pending& p) { params_on_side(*p.r, p.d); }); }
    void params_on_side(const HRec& r, const h16* d)
    {
        const Layer& l = *r.l;
        hipStream_t s2 = sq.side ? sq.side : st;
        if (l.has_bias && l.bn.empty()) {                        // a bias in front of a train-mode BatchNorm has an exactly zero gradient
            HRedArgs q{};
            q.y = d; q.y_ld = r.Np; q.y_off = 0; q.M = (int)r.Mo; q.C = r.oC; q.Cp = r.Np; q.half = r.ohalf; q.gap = r.ogap;
            q.facc = GS(l.conv + ".bias"); q.slot_stride = (size_t)h->tN;
            launch_hcol_reduce(q, 3, s2);
        }
        if (l.kind == K_PW || l.kind == K_DENSE3) {
            HWgradArgs a{};
            a.dy = d; a.dy_ld = r.Np; a.x = r.x.p; a.x_ld = r.x.ld; a.x_off = r.x.off; a.H = r.H; a.W = r.W; a.taps = l.kind == K_DENSE3 ? 9 : 1;
            a.M = (int)r.Mo; a.Np = r.Np; a.Kp = r.x.Cp; a.N = l.cout; a.Cin = l.cin; a.half = r.x.half; a.gap = r.x.gap;
            a.dw = G(l.conv + ".weight"); a.partial = sc.wpart; a.partial_cap = sc.wpart_cap;
            launch_hwgrad(a, s2);
        } else if (l.kind == K_DW) {
            launch_hdw_wgrad(d, r.Np, r.x.p, r.x.ld, r.x.off, r.B, r.H, r.W, r.oC, r.Np, r.ohalf, r.ogap, l.stride, GS(l.conv + ".weight"), sc.wpart, sc.wpart_cap, s2);
        } else {
            launch_hstem_wgrad(d, r.x_nchw, r.B, r.H, r.W, GS(l.conv + ".weight"), (size_t)h->tN, s2);
        }
    }
    // this launch writes the COMPLETE dz of layer `below`: its BatchNorm-backward sums on the way (the launch's HColStat epilogue)
    void sums_below(HColStat& s, int below, const HRec& r, const HV& dx)
    {
        if (below < 0 || !sw.fuse_sums || dx.off != 0) return;
        HRec& b = recs[below];
        const Layer& bl = *b.l;
        if (!b.acc || b.Mo != r.Mi || b.Np != dx.Cp) return;
        s.acc = b.acc + 2 * HACC_SLOTS * (size_t)bl.cout; s.C = b.oC; s.half = b.ohalf; s.gap = b.ogap;
        s.y = b.y; s.y_ld = b.Np; s.mean = b.mean; s.invstd = b.invstd; s.gamma = P(bl.bn + ".weight"); s.beta = P(bl.bn + ".bias"); s.act = bl.act;
        b.sums_done = true;
    }
    // gradient w.r.t. the conv input, written (or accumulated) into the view dx (same geometry as r.x)
    // below >= 0: dx is the COMPLETE gradient of layer recs[below]'s BN + activation output (this conv is its only consumer): its
    // BatchNorm-backward sums are taken in this kernel's epilogue
    void back_input(const HRec& r, const h16* d, HV dx, bool accumulate, int below = -1)
    {
        const Layer& l = *r.l;
        const HPack& pk = pack(l);
        if (l.kind == K_DW && l.stride == 2) {
            launch_hdw_dgrad_s2(d, r.Np, pk.dwf, r.B, r.H, r.W, r.Np, dx.p, dx.ld, dx.off, accumulate ? 1 : 0, st);
        } else if (l.kind == K_DW) {
            HDwArgs a{};
            a.in = d; a.in_ld = r.Np; a.in_off = 0; a.w = pk.dwb; a.bias = nullptr; a.out = dx.p; a.out_ld = dx.ld; a.out_off = dx.off;
            a.B = r.B; a.H = r.H; a.W = r.W; a.Cp = r.Np; a.stride = 1; a.accumulate = accumulate ? 1 : 0;
            if (!accumulate && r.Np <= 256 && dx.ld == dx.Cp) sums_below(a.st, below, r, dx);
            launch_hdw(a, st);
        } else {
            HGemmArgs a{};
            a.in = d; a.in_ld = r.Np; a.in_off = 0; a.H = r.H; a.W = r.W; a.taps = l.kind == K_DENSE3 ? 9 : 1;
            a.Wp = pk.wb; a.bias = nullptr; a.out = dx.p; a.out_ld = dx.ld; a.out_off = dx.off;
            a.M = (int)r.Mo; a.Kp = pk.Kpb; a.Np = dx.Cp; a.Npad = pk.Npadb; a.accumulate = accumulate ? 1 : 0;
            if (!accumulate) sums_below(a.st, below, r, dx);
            launch_hgemm(a, st);
        }
    }
    void back(int ri, HV dz, HV dx, bool accumulate, bool need_input = true, int below = -1)
    {
        const h16* d = back_params(recs[ri], dz, nullptr, nullptr);
        if (need_input) back_input(recs[ri], d, dx, accumulate, below);
    }
    // pw2's backward from the odd channels of the unit's output gradient; hbn_bwd_kernel writes the even (pass-through) half to even_dst on
    // its way (it loads those values anyway) when the layer has a BatchNorm - else (false) the half is gathered by a launch of its own
    bool back_unit_s2(int ri, const HTen& unit, HV dx, HV even_dst, int below)
    {
        const bool fused = !recs[ri].l->bn.empty();
        const h16* d = back_params(recs[ri], HV{}, &unit, &even_dst);
        back_input(recs[ri], d, dx, false, below);
        return fused;
    }
    void back_unit_s1(int ri, const HTen& unit, HV dx, HV even_dst, int below) { if (!back_unit_s2(ri, unit, dx, even_dst, below)) even_to(unit, even_dst); }
    void even_to(const HTen& unit, HV dst) { launch_hgather(unit.g, unit.Cp, 0, 2, unit.half, unit.gap, dst.p, dst.ld, dst.off, 1, dst.half, dst.gap, unit.M, unit.half, dst.Cp, st); }
};

}  // namespace
