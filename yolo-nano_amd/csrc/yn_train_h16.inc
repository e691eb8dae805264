// yn_train_h16.inc — the training step of yn_train.inc in mixed precision (BASELINE configs[2]: "SGD training step fp16"),
// included by yn_api.hip after yn_train.inc.  Same tape, same wiring (train.py:219-231; models/yolo_nano.py:282-358;
// backbone/shufflenetv2.py:69-78), different arithmetic: fp16 storage of activations / activation gradients in the
// channel-padded layout of kernels_h16.hip, f16 MFMA with fp32 accumulation for every GEMM-shaped conv, fp32 master weights
// (the caller's flat buffers, unchanged), fp32 BatchNorm statistics / parameter gradients, dynamic loss scale on the device.
// yn_train_step dispatches here when yn_train_precision(h, YN_F16) was called.

namespace {

// zero-filled scratch of the op-level entry points (yn_op_h16_*), freed on scope exit
struct DevBuf {
    void* p = nullptr;
    explicit DevBuf(size_t bytes, hipStream_t st) { if (hipMalloc(&p, bytes ? bytes : 16) == hipSuccess) (void)hipMemsetAsync(p, 0, bytes ? bytes : 16, st); else p = nullptr; }
    ~DevBuf() { if (p) (void)hipFree(p); }
    template <class T> T* as() { return (T*)p; }
};

inline int r8(int c) { return (c + 7) & ~7; }
inline int r32(int c) { return (c + 31) & ~31; }

struct HTen { h16* v; h16* g; long M; int C, Cp, half, gap; };                 // value + gradient, channel map (kernels_h16.hip)
struct HV { h16* p; int ld, off, C, Cp, half, gap; };                          // view: C logical channels in Cp physical ones starting at off
inline HV vfull(const HTen& t, bool grad = false) { return HV{grad ? t.g : t.v, t.Cp, 0, t.C, t.Cp, t.half, t.gap}; }
// one plane of a gapped unit tensor: x1 = logical [0, bf), x2 = logical [bf, 2bf)
inline HV vplane(const HTen& t, int which, bool grad = false) { return HV{grad ? t.g : t.v, t.Cp, which ? t.half + t.gap : 0, t.half, t.half + t.gap, t.half, 0}; }

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

struct HTrainer {
    yn_handle* h;
    int B, S;
    hipStream_t st;
    char* base; size_t used = 0, cap;
    size_t gused = 0;
    std::vector<HRec> recs;
    bool fuse_stats = true, fuse_sums = true;                                   // HColStat epilogues (YN_TRAIN_FUSE_STATS / YN_TRAIN_FUSE_SUMS = 0: separate reduction launches)
    h16* even_dst = nullptr; int even_ld = 0; bool even_done = false;         // back(): also extract the unit gradient's even channels (set by the caller per call)
    // The weight gradients run on a second stream.  A layer's BatchNorm backward writes dy IN PLACE over the pre-BN conv output y (nothing
    // reads y afterwards), so no buffer is ever reused and the side stream only ever has to wait for the main one: one event per BATCH of
    // layers (an event record costs the main stream 7 us of idle queue before its next kernel: 1.2 ms per step with one per layer).
    static constexpr int NEV = 32, BATCH = 4;
    hipStream_t side = nullptr;
    hipEvent_t ev[NEV];
    int ei = 0;
    struct Pending { const HRec* r; const h16* d; };
    std::vector<Pending> pending;
    double* stats = nullptr; size_t stats_used = 0, stats_cap = 0;
    float* wpart = nullptr; size_t wpart_cap = 0;
    float* gslots = nullptr;
    bool oom = false;

    void* take_b(size_t bytes)
    {
        bytes = (bytes + 255) & ~(size_t)255;
        if (used + bytes + gused > cap) { oom = true; return base; }
        void* p = base + used;
        used += bytes;
        return p;
    }
    h16* take(size_t halves) { return (h16*)take_b(halves * sizeof(h16)); }
    h16* take_g(size_t halves)
    {
        const size_t bytes = (halves * sizeof(h16) + 255) & ~(size_t)255;
        if (used + bytes + gused > cap) { oom = true; return (h16*)base; }
        gused += bytes;
        return (h16*)(base + cap - gused);
    }
    HTen mk(long M, int C) { return HTen{take((size_t)M * r8(C)), take_g((size_t)M * r8(C)), M, C, r8(C), C, 0}; }
    HTen mk_unit(long M, int bf) { const int bfp = r8(bf); return HTen{take((size_t)M * 2 * bfp), take_g((size_t)M * 2 * bfp), M, 2 * bf, 2 * bfp, bf, bfp - bf}; }
    float* P(const std::string& k) { return h->tP + h->toff.at(k); }
    float* G(const std::string& k) { return h->tG + h->toff.at(k); }
    float* GS(const std::string& k) { return gslots + h->toff.at(k); }
    HPack& pack(const Layer& l) { return h->hpacks[(size_t)(&l - &h->layers[0])]; }

    // (re)build the layer's packs from the fp32 master weights for the channel map of its input view
    int prepare(const Layer& l, const HV& x)
    {
        if (h->hpack_table) return 0;                        // steady state: every pack was rebuilt by ONE launch at the start of the step
        HPack& pk = pack(l);
        const float* w = P(l.conv + ".weight");
        const float* b = l.has_bias ? P(l.conv + ".bias") : nullptr;
        if (l.kind == K_DW) {
            if (!pk.dwf) {
                if (hipMalloc((void**)&pk.dwf, (size_t)9 * x.Cp * sizeof(float)) != hipSuccess || hipMalloc((void**)&pk.dwb, (size_t)9 * x.Cp * sizeof(float)) != hipSuccess ||
                    hipMalloc((void**)&pk.bias, (size_t)x.Cp * sizeof(float)) != hipSuccess) return 1;
                (void)hipMemsetAsync(pk.dwf, 0, (size_t)9 * x.Cp * sizeof(float), st);
                (void)hipMemsetAsync(pk.dwb, 0, (size_t)9 * x.Cp * sizeof(float), st);
                (void)hipMemsetAsync(pk.bias, 0, (size_t)x.Cp * sizeof(float), st);
                pk.Kp = x.Cp;
            }
            launch_hpack_dw(w, b, l.cout, x.half, x.gap, x.Cp, 0, pk.dwf, pk.bias, st);
            if (l.stride == 1) launch_hpack_dw(w, nullptr, l.cout, x.half, x.gap, x.Cp, 1, pk.dwb, nullptr, st);
            h->hpack_jobs.push_back(HPackDesc{w, b, 1, l.cout, l.cin, 9, x.half, x.gap, x.Cp, 0, 0, 0, nullptr, nullptr, pk.bias, pk.dwf, l.stride == 1 ? pk.dwb : nullptr});
        } else if (l.kind == K_STEM) {
            if (!pk.dwf) { if (hipMalloc((void**)&pk.dwf, (size_t)27 * 24 * sizeof(float)) != hipSuccess) return 1; }
            launch_hpack_stem(w, pk.dwf, st);
            h->hpack_jobs.push_back(HPackDesc{w, nullptr, 2, 24, 3, 9, 3, 0, 0, 0, 0, 0, nullptr, nullptr, nullptr, pk.dwf, nullptr});
        } else {
            const int taps = l.kind == K_DENSE3 ? 9 : 1;
            if (!pk.wf) {
                pk.Kp = x.Cp; pk.Npad = r32(l.cout); pk.Kpb = r8(l.cout); pk.Npadb = r32(x.Cp);
                const size_t nf = (size_t)taps * pk.Kp * pk.Npad, nb = (size_t)taps * pk.Kpb * pk.Npadb;
                if (hipMalloc((void**)&pk.wf, nf * sizeof(h16)) != hipSuccess || hipMalloc((void**)&pk.wb, nb * sizeof(h16)) != hipSuccess ||
                    hipMalloc((void**)&pk.bias, (size_t)pk.Npad * sizeof(float)) != hipSuccess) return 1;
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
            r.mean = (float*)take_b((size_t)l.cout * sizeof(float)); r.invstd = (float*)take_b((size_t)l.cout * sizeof(float));
            if (stats_used + 4 * HACC_SLOTS * (size_t)l.cout > stats_cap) { oom = true; recs.push_back(r); return (int)recs.size() - 1; }
            r.acc = stats + stats_used; stats_used += 4 * HACC_SLOTS * (size_t)l.cout;
        }
        if (prepare(l, x)) { oom = true; recs.push_back(r); return (int)recs.size() - 1; }
        const HPack& pk = pack(l);
        if (l.kind == K_PW || l.kind == K_DENSE3) {
            HGemmArgs a{};
            a.in = x.p; a.in_ld = x.ld; a.in_off = x.off; a.H = H; a.W = W; a.taps = l.kind == K_DENSE3 ? 9 : 1;
            a.Wp = pk.wf; a.bias = pk.bias; a.out = r.y; a.out_ld = r.Np; a.out_off = 0;
            a.M = (int)r.Mo; a.Kp = pk.Kp; a.Np = r.Np; a.Npad = pk.Npad; a.accumulate = 0;
            if (r.acc && fuse_stats) { a.st.acc = r.acc; a.st.C = r.oC; a.st.half = r.ohalf; a.st.gap = r.ogap; r.stats_done = true; }      // BatchNorm statistics in the epilogue
            launch_hgemm(a, st);
        } else if (l.kind == K_DW) {
            HDwArgs a{};
            a.in = x.p; a.in_ld = x.ld; a.in_off = x.off; a.w = pk.dwf; a.bias = pk.bias; a.out = r.y; a.out_ld = r.Np; a.out_off = 0;
            a.B = B_; a.H = H; a.W = W; a.Cp = x.Cp; a.stride = l.stride; a.accumulate = 0;
            if (r.acc && fuse_stats && l.stride == 1 && x.Cp <= 256) { a.st.acc = r.acc; a.st.C = r.oC; a.st.half = r.ohalf; a.st.gap = r.ogap; r.stats_done = true; }   // statistics in the run kernel's epilogue
            launch_hdw(a, st);
        } else {
            launch_hstem(x_nchw, B_, H, W, pk.dwf, nullptr, r.y, st);
        }
        recs.push_back(r);
        return (int)recs.size() - 1;
    }
    // BatchNorm (batch statistics) + activation: dense into `out` (same channel map as the conv output), or — pass != null —
    // the concat+shuffle of a ShuffleV2 unit into the gapped tensor `unit`: unit[2c] = pass[c], unit[2c+1] = z[c]
    void bn(int ri, h16* out, int out_ld, int out_off, const HV* pass = nullptr, const HTen* unit = nullptr)
    {
        HRec& r = recs[ri];
        const Layer& l = *r.l;
        if (!r.acc) { oom = true; return; }
        const Param* rm = find_param(h, l.bn + ".running_mean");
        const Param* rv = find_param(h, l.bn + ".running_var");
        HRedArgs q{};
        q.y = r.y; q.y_ld = r.Np; q.y_off = 0; q.M = (int)r.Mo; q.C = r.oC; q.Cp = r.Np; q.half = r.ohalf; q.gap = r.ogap; q.acc = r.acc;
        if (!r.stats_done) launch_hcol_reduce(q, 0, st);
        HBnApplyArgs a{};
        a.y = r.y; a.y_ld = r.Np; a.acc = r.acc; a.eps = 1e-5f; a.M = (int)r.Mo; a.C = r.oC; a.Cp = r.Np; a.half = r.ohalf; a.gap = r.ogap; a.act = l.act;
        a.mean = r.mean; a.invstd = r.invstd; a.gamma = P(l.bn + ".weight"); a.beta = P(l.bn + ".bias");
        a.rmean = rm ? (float*)rm->dev : nullptr; a.rvar = rv ? (float*)rv->dev : nullptr; a.momentum = 0.1f;
        if (pass) { a.out = unit->v; a.out_ld = unit->Cp; a.out_off = 0; a.pass = pass->p; a.pass_ld = pass->ld; a.pass_off = pass->off; a.out_half = unit->half; a.out_gap = unit->gap; }
        else { a.out = out; a.out_ld = out_ld; a.out_off = out_off; }
        launch_hbn_apply(a, st);
    }

    // the stem: BatchNorm (statistics taken here when the conv did not) + activation + 3x3 / 2 max pool -> a1, arg-max positions
    void stem_pool(int ri, int B_, int H1, h16* out, uint8_t* idx)
    {
        HRec& r = recs[ri];
        const Layer& l = *r.l;
        if (!r.acc) { oom = true; return; }
        const Param* rm = find_param(h, l.bn + ".running_mean");
        const Param* rv = find_param(h, l.bn + ".running_var");
        HRedArgs q{};
        q.y = r.y; q.y_ld = r.Np; q.y_off = 0; q.M = (int)r.Mo; q.C = r.oC; q.Cp = r.Np; q.half = r.ohalf; q.gap = r.ogap; q.acc = r.acc;
        if (!r.stats_done) launch_hcol_reduce(q, 0, st);
        HBnApplyArgs a{};
        a.y = r.y; a.y_ld = r.Np; a.acc = r.acc; a.eps = 1e-5f; a.M = (int)r.Mo; a.C = r.oC; a.Cp = r.Np; a.half = r.ohalf; a.gap = r.ogap; a.act = l.act;
        a.mean = r.mean; a.invstd = r.invstd; a.gamma = P(l.bn + ".weight"); a.beta = P(l.bn + ".bias");
        a.rmean = rm ? (float*)rm->dev : nullptr; a.rvar = rv ? (float*)rv->dev : nullptr; a.momentum = 0.1f;
        launch_hstem_apply_pool(a, B_, H1, H1, out, idx, st);
    }
    // ... and its way back: the pool's gather feeds the BatchNorm-backward sums and the in-place dy directly; then the stem conv's weight gradient
    void back_stem(int ri, const h16* pool_grad, const uint8_t* idx, int B_, int H1)
    {
        const HRec& r = recs[ri];
        const Layer& l = *r.l;
        HRedArgs q{};
        q.y = r.y; q.y_ld = r.Np; q.y_off = 0; q.M = (int)r.Mo; q.C = r.oC; q.Cp = r.Np; q.half = r.ohalf; q.gap = r.ogap;
        q.mean = r.mean; q.invstd = r.invstd; q.gamma = P(l.bn + ".weight"); q.beta = P(l.bn + ".bias"); q.act = l.act;
        q.acc = r.acc + 2 * HACC_SLOTS * (size_t)l.cout;
        launch_hstem_bwd(q, pool_grad, idx, B_, H1, H1, r.y, G(l.bn + ".weight"), G(l.bn + ".bias"), st);
        if (!side) { params_on_side(r, r.y); return; }
        pending.push_back(Pending{&r, r.y});
        if ((int)pending.size() >= BATCH) flush_params();
    }

    // ---- backward pieces ----
    // dz: gradient of the layer's BN+act output — a dense view with the conv output's map, or (odd_of != null) the odd logical
    // channels of the gapped unit gradient.  Returns dy (dense [Mo][Np]).
    const h16* back_params(const HRec& r, const h16* dz, int dz_ld, int dz_off, const HTen* odd_of)
    {
        const Layer& l = *r.l;
        const h16* d;
        if (!l.bn.empty()) {
            h16* dy = r.y;                                        // in place
            HRedArgs q{};
            q.y = r.y; q.y_ld = r.Np; q.y_off = 0; q.M = (int)r.Mo; q.C = r.oC; q.Cp = r.Np; q.half = r.ohalf; q.gap = r.ogap;
            if (odd_of) { q.dz = odd_of->g; q.dz_ld = odd_of->Cp; q.dz_off = 0; q.dz_odd = 1; q.dz_half = odd_of->half; q.dz_gap = odd_of->gap; }
            else { q.dz = dz; q.dz_ld = dz_ld; q.dz_off = dz_off; q.dz_odd = 0; }
            q.mean = r.mean; q.invstd = r.invstd; q.gamma = P(l.bn + ".weight"); q.beta = P(l.bn + ".bias"); q.act = l.act;
            q.acc = r.acc + 2 * HACC_SLOTS * (size_t)l.cout;
            if (odd_of && even_dst) { q.even = even_dst; q.even_ld = even_ld; even_done = true; }     // the pass-through half leaves with the same loads
            launch_hbn_bwd(q, dy, G(l.bn + ".weight"), G(l.bn + ".bias"), st, r.sums_done);
            d = dy;
        } else {
            d = dz + dz_off;                                      // plain conv output (head): dense [Mo][Np]
        }
        if (!side) { params_on_side(r, d); return d; }
        pending.push_back(Pending{&r, d});
        if ((int)pending.size() >= BATCH) flush_params();
        return d;
    }
    // everything queued so far is complete on the main stream after this point: hand it to the side stream
    void flush_params()
    {
        if (pending.empty()) return;
        if (side) {
            hipEvent_t e = ev[ei++ % NEV];
            (void)hipEventRecord(e, st);
            (void)hipStreamWaitEvent(side, e, 0);
        }
        for (const Pending& p : pending) params_on_side(*p.r, p.d);
        pending.clear();
    }
    void params_on_side(const HRec& r, const h16* d)
    {
        const Layer& l = *r.l;
        hipStream_t s2 = side ? side : st;
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
            a.dw = G(l.conv + ".weight"); a.partial = wpart; a.partial_cap = wpart_cap;
            launch_hwgrad(a, s2);
        } else if (l.kind == K_DW) {
            launch_hdw_wgrad(d, r.Np, r.x.p, r.x.ld, r.x.off, r.B, r.H, r.W, r.oC, r.Np, r.ohalf, r.ogap, l.stride, GS(l.conv + ".weight"), wpart, wpart_cap, s2);
        } else {
            launch_hstem_wgrad(d, r.x_nchw, r.B, r.H, r.W, GS(l.conv + ".weight"), (size_t)h->tN, s2);
        }
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
            if (below >= 0 && fuse_sums && !accumulate && dx.off == 0 && r.Np <= 256) {       // this launch writes the COMPLETE dz of layer `below`: its BatchNorm-backward sums on the way
                HRec& b = recs[below];
                const Layer& bl = *b.l;
                if (b.acc && b.Mo == r.Mi && b.Np == dx.Cp && dx.ld == dx.Cp) {
                    a.st.acc = b.acc + 2 * HACC_SLOTS * (size_t)bl.cout; a.st.C = b.oC; a.st.half = b.ohalf; a.st.gap = b.ogap;
                    a.st.y = b.y; a.st.y_ld = b.Np; a.st.mean = b.mean; a.st.invstd = b.invstd; a.st.gamma = P(bl.bn + ".weight"); a.st.beta = P(bl.bn + ".bias"); a.st.act = bl.act;
                    b.sums_done = true;
                }
            }
            launch_hdw(a, st);
        } else {
            HGemmArgs a{};
            a.in = d; a.in_ld = r.Np; a.in_off = 0; a.H = r.H; a.W = r.W; a.taps = l.kind == K_DENSE3 ? 9 : 1;
            a.Wp = pk.wb; a.bias = nullptr; a.out = dx.p; a.out_ld = dx.ld; a.out_off = dx.off;
            a.M = (int)r.Mo; a.Kp = pk.Kpb; a.Np = dx.Cp; a.Npad = pk.Npadb; a.accumulate = accumulate ? 1 : 0;
            if (below >= 0 && fuse_sums && !accumulate && dx.off == 0) {
                HRec& b = recs[below];
                const Layer& bl = *b.l;
                if (b.acc && b.Mo == r.Mi && b.Np == dx.Cp) {
                    a.st.acc = b.acc + 2 * HACC_SLOTS * (size_t)bl.cout; a.st.C = b.oC; a.st.half = b.ohalf; a.st.gap = b.ogap;
                    a.st.y = b.y; a.st.y_ld = b.Np; a.st.mean = b.mean; a.st.invstd = b.invstd; a.st.gamma = P(bl.bn + ".weight"); a.st.beta = P(bl.bn + ".bias"); a.st.act = bl.act;
                    b.sums_done = true;
                }
            }
            launch_hgemm(a, st);
        }
    }
    void back(int ri, const h16* dz, int dz_ld, int dz_off, const HTen* odd_of, HV dx, bool accumulate, bool need_input = true, int below = -1)
    {
        const h16* d = back_params(recs[ri], dz, dz_ld, dz_off, odd_of);
        if (need_input) back_input(recs[ri], d, dx, accumulate, below);
    }
    void back_dense(int ri, const HTen& out, HV dx, bool accumulate, bool need_input = true, int below = -1) { back(ri, out.g, out.Cp, 0, nullptr, dx, accumulate, need_input, below); }
};

// Everything of the step between the host-side preparation and the optimiser: loss-scale settlement, weight packs, forward, loss, backward,
// gradient combine.  No allocation, no synchronisation, the same launches with the same arguments for the same (x, target, losses, B, S):
// the part train_step_h16 captures into a hipGraph.
int train_body_h16(yn_handle* h, const float* x_dev, const float* target_dev, int B, float* losses_dev)
{
    const int S = h->grid.S;
    hipStream_t st = h->stream;
    launch_hscale_update(h->scale_state, nullptr, st);     // a previous step nobody ran yn_sgd_step for: settle its scale decision from the local flag
    HTrainer T{h, B, S, st, h->train_arena, 0, h->train_arena_bytes};
    T.recs.reserve(h->layers.size() + 4);
    const int HCp = r8(h->head_ch);
    if (h->multi_stream && !h->profiling && h->train_side && h->train_events.size() >= (size_t)HTrainer::NEV + 1) {
        T.side = h->train_side;
        for (int i = 0; i < HTrainer::NEV; ++i) T.ev[i] = h->train_events[i];
    }
    {
        // (read at every step, not once per process: the tests compare the two forms of a step inside one process)
        const int fs = getenv("YN_TRAIN_FUSE_STATS") ? atoi(getenv("YN_TRAIN_FUSE_STATS")) : 1, fb = getenv("YN_TRAIN_FUSE_SUMS") ? atoi(getenv("YN_TRAIN_FUSE_SUMS")) : 1;
        T.fuse_stats = fs != 0; T.fuse_sums = fb != 0;
    }
    {
        size_t nstat = 0;
        for (const Layer& l : h->layers) if (!l.bn.empty()) nstat += 4 * HACC_SLOTS * (size_t)l.cout;
        T.stats = (double*)T.take_b(nstat * sizeof(double));
        T.stats_cap = nstat;
        HIPCHK(h, hipMemsetAsync(T.stats, 0, nstat * sizeof(double), st));
        T.wpart_cap = (size_t)16 << 20;
        T.wpart = (float*)T.take_b(T.wpart_cap * sizeof(float));
        T.gslots = (float*)T.take_b((size_t)GRAD_SLOTS * h->tN * sizeof(float));
        HIPCHK(h, hipMemsetAsync(T.gslots, 0, (size_t)GRAD_SLOTS * h->tN * sizeof(float), st));
    }
    HIPCHK(h, hipMemsetAsync(h->tG, 0, h->tN * sizeof(float), st));
    if (h->hpack_table) launch_hpack_all(h->hpack_table, h->hpack_table_n, st);          // all weight packs from the current master weights

    // =============================== forward (train mode) ===============================
    const int H1 = S / 2, H2 = S / 4;
    const long M1 = (long)B * H1 * H1, M2 = (long)B * H2 * H2;
    // the stem's BatchNorm + activation + max pool as one kernel, its backward without the full-resolution gradient (kernels_h16.hip,
    // hstem_apply_pool_kernel / hstem_bwd_kernel; YN_TRAIN_STEM_FUSE=0: the separate launches, for the tests)
    const bool stem_fuse = !(getenv("YN_TRAIN_STEM_FUSE") && atoi(getenv("YN_TRAIN_STEM_FUSE")) == 0);
    HTen a0{}, a1 = T.mk(M2, 24);
    if (!stem_fuse) a0 = T.mk(M1, 24);
    uint8_t* pool_idx = (uint8_t*)T.take_b((size_t)M2 * 24);
    const int r_stem = T.conv(L(h, "stem"), HV{nullptr, 0, 0, 3, 8, 3, 0}, B, S, S, x_dev);
    if (stem_fuse) T.stem_pool(r_stem, B, H1, a1.v, pool_idx);
    else {
        T.bn(r_stem, a0.v, a0.Cp, 0);
        launch_hmaxpool_idx(a0.v, B, H1, H1, 24, a1.v, pool_idx, st);
    }

    struct Blk { int s2; int r_b1dw, r_b1pw, r_pw1, r_dw, r_pw2; HTen in, tdw1, tb1, t1, t2, out; int Hin, Hout, Cin, C, bf; };
    std::vector<Blk> blks;
    HTen cur = a1;
    int curH = H2;
    HTen cfeat[3];
    char nm[96];
    for (int si = 0; si < 3; ++si) {
        const int C = h->stage_ch[si], bf = C / 2;
        for (int bi = 0; bi < STAGE_REP[si]; ++bi) {
            snprintf(nm, sizeof nm, "backbone.stage%d.%d", si + 2, bi);
            const std::string Pn = nm;
            Blk k{};
            k.in = cur; k.Cin = cur.C; k.C = C; k.bf = bf; k.Hin = curH;
            if (bi == 0) {
                const int Ho = curH / 2;
                const long Mi = (long)B * curH * curH, Mo = (long)B * Ho * Ho;
                k.s2 = 1; k.Hout = Ho;
                k.tdw1 = HTen{T.take((size_t)Mo * cur.Cp), T.take_g((size_t)Mo * cur.Cp), Mo, cur.C, cur.Cp, cur.half, cur.gap};     // channel-wise: the input's map
                k.tb1 = T.mk(Mo, bf); k.t1 = T.mk(Mi, bf); k.t2 = T.mk(Mo, bf); k.out = T.mk_unit(Mo, bf);
                k.r_b1dw = T.conv(L(h, Pn + ".b1.dw"), vfull(cur), B, curH, curH); T.bn(k.r_b1dw, k.tdw1.v, k.tdw1.Cp, 0);
                k.r_b1pw = T.conv(L(h, Pn + ".b1.pw"), vfull(k.tdw1), B, Ho, Ho); T.bn(k.r_b1pw, k.tb1.v, k.tb1.Cp, 0);
                k.r_pw1 = T.conv(L(h, Pn + ".b2.pw1"), vfull(cur), B, curH, curH); T.bn(k.r_pw1, k.t1.v, k.t1.Cp, 0);
                k.r_dw = T.conv(L(h, Pn + ".b2.dw"), vfull(k.t1), B, curH, curH); T.bn(k.r_dw, k.t2.v, k.t2.Cp, 0);
                k.r_pw2 = T.conv(L(h, Pn + ".b2.pw2"), vfull(k.t2), B, Ho, Ho);
                { const HV pass = vfull(k.tb1); T.bn(k.r_pw2, nullptr, 0, 0, &pass, &k.out); }           // out[2j] = b1[j], out[2j+1] = b2[j]
                curH = Ho;
            } else {
                const long Mo = (long)B * curH * curH;
                k.s2 = 0; k.Hout = curH;
                k.t1 = T.mk(Mo, bf); k.t2 = T.mk(Mo, bf); k.out = T.mk_unit(Mo, bf);
                k.r_pw1 = T.conv(L(h, Pn + ".b2.pw1"), vplane(cur, 1), B, curH, curH); T.bn(k.r_pw1, k.t1.v, k.t1.Cp, 0);
                k.r_dw = T.conv(L(h, Pn + ".b2.dw"), vfull(k.t1), B, curH, curH); T.bn(k.r_dw, k.t2.v, k.t2.Cp, 0);
                k.r_pw2 = T.conv(L(h, Pn + ".b2.pw2"), vfull(k.t2), B, curH, curH);
                { const HV pass = vplane(cur, 0); T.bn(k.r_pw2, nullptr, 0, 0, &pass, &k.out); }          // out[2j] = x1[j]
            }
            cur = k.out;
            blks.push_back(k);
        }
        cfeat[si] = cur;
    }
    // neck
    const int W3 = S / 8, W4 = S / 16, W5 = S / 32;
    const long M3 = (long)B * W3 * W3, M4 = (long)B * W4 * W4, M5 = (long)B * W5 * W5;
    HTen p3 = T.mk(M3, NECK), p4 = T.mk(M4, NECK), p5 = T.mk(M5, NECK);
    HTen u4 = T.mk(M4, NECK), p4a = T.mk(M4, NECK), u3 = T.mk(M3, NECK), p3a = T.mk(M3, NECK), d4 = T.mk(M4, NECK), p4b = T.mk(M4, NECK), d5 = T.mk(M5, NECK), p5a = T.mk(M5, NECK);
    // u = p + up2(q) / d = p + down(q): the gradient of the sum IS the gradient of its same-resolution term, so the two share one buffer
    // (the sum's gradient has been consumed by the time the term's other contributions are accumulated into it): four device copies less
    p5.g = d5.g; p4a.g = d4.g; p3.g = u3.g; p4.g = u4.g;
    const int r_lat0 = T.conv(L(h, "conv1x1_0"), vfull(cfeat[0]), B, W3, W3); T.bn(r_lat0, p3.v, NECK, 0);
    const int r_lat1 = T.conv(L(h, "conv1x1_1"), vfull(cfeat[1]), B, W4, W4); T.bn(r_lat1, p4.v, NECK, 0);
    const int r_lat2 = T.conv(L(h, "conv1x1_2"), vfull(cfeat[2]), B, W5, W5); T.bn(r_lat2, p5.v, NECK, 0);
    launch_hresample(p4.v, p5.v, u4.v, B, W4, W4, NECK, 0, st);
    const int r_sm0 = T.conv(L(h, "smooth_0"), vfull(u4), B, W4, W4); T.bn(r_sm0, p4a.v, NECK, 0);
    // The three head towers are independent chains of small kernels (19x19 / 38x38 maps: 6-10 us launches that fill a fraction of the chip):
    // level 3 starts on a fork stream as soon as smooth_1 is done and runs beside the rest of the neck, level 4 on a second one, level 5
    // stays on the main stream; all join before the loss.  (Backward: the same towers fork again after the loss.)
    HTen feats[3] = {p3a, p4b, p5a};
    const int Ws[3] = {W3, W4, W5};
    struct HeadT { HTen t[4]; int r[5]; h16* out; h16* gout; long M; };
    HeadT hd[3];
    // the three raw-head gradients in ONE block (one memset before the loss instead of three)
    const size_t gout_off[3] = {0, (size_t)M3 * HCp, (size_t)(M3 + M4) * HCp};
    const size_t gout_total = (size_t)(M3 + M4 + M5) * HCp;
    h16* gout_all = T.take_g(gout_total);
    hipStream_t fk[2] = {nullptr, nullptr};
    hipEvent_t fev[8];
    if (T.side && h->train_fork[0] && h->train_fork[1] && h->train_events.size() >= (size_t)HTrainer::NEV + 9) {
        if (h->head_fork_now) { fk[0] = h->train_fork[0]; fk[1] = h->train_fork[1]; }
        for (int i = 0; i < 8; ++i) fev[i] = h->train_events[HTrainer::NEV + 1 + i];
    }
    auto head_fwd = [&](int k, hipStream_t on, hipEvent_t e_fork) {
        if (on) { (void)hipEventRecord(e_fork, st); (void)hipStreamWaitEvent(on, e_fork, 0); T.st = on; }
        const long M = (long)B * Ws[k] * Ws[k];
        char hn[64];
        snprintf(hn, sizeof hn, "head_det_%d", k + 1);
        const std::string Pn = hn;
        hd[k].M = M;
        for (int j = 0; j < 4; ++j) hd[k].t[j] = T.mk(M, NECK);
        HTen in = feats[k];
        for (int j = 0; j < 4; ++j) {
            hd[k].r[j] = T.conv(L(h, Pn + "." + std::to_string(j)), vfull(in), B, Ws[k], Ws[k]);
            T.bn(hd[k].r[j], hd[k].t[j].v, NECK, 0);
            in = hd[k].t[j];
        }
        hd[k].r[4] = T.conv(L(h, Pn + ".4"), vfull(in), B, Ws[k], Ws[k]);       // plain conv + bias, no BN: its output IS the raw head [M][HCp]
        hd[k].out = T.recs[hd[k].r[4]].y;
        hd[k].gout = gout_all + gout_off[k];
        T.st = st;
    };
    launch_hresample(p3.v, p4a.v, u3.v, B, W3, W3, NECK, 0, st);
    const int r_sm1 = T.conv(L(h, "smooth_1"), vfull(u3), B, W3, W3); T.bn(r_sm1, p3a.v, NECK, 0);
    launch_hresample(p4a.v, p3a.v, d4.v, B, W4, W4, NECK, 1, st);
    head_fwd(0, fk[0], fev[0]);                                                  // (after the resample that also reads p3a: one event covers both)
    const int r_sm2 = T.conv(L(h, "smooth_2"), vfull(d4), B, W4, W4); T.bn(r_sm2, p4b.v, NECK, 0);
    launch_hresample(p5.v, p4b.v, d5.v, B, W5, W5, NECK, 1, st);
    head_fwd(1, fk[1], fev[1]);
    const int r_sm3 = T.conv(L(h, "smooth_3"), vfull(d5), B, W5, W5); T.bn(r_sm3, p5a.v, NECK, 0);
    head_fwd(2, nullptr, nullptr);
    for (int i = 0; i < 2; ++i)
        if (fk[i]) { (void)hipEventRecord(fev[2 + i], fk[i]); (void)hipStreamWaitEvent(st, fev[2 + i], 0); }
    if (T.oom) return fail(h, "training workspace exhausted (%zu bytes)", h->train_arena_bytes);
    if (!h->hpack_table && !h->hpack_jobs.empty()) {       // the first step packed layer by layer and recorded the jobs: upload the table
        HIPCHK(h, hipMalloc((void**)&h->hpack_table, h->hpack_jobs.size() * sizeof(HPackDesc)));
        HIPCHK(h, hipMemcpyAsync(h->hpack_table, h->hpack_jobs.data(), h->hpack_jobs.size() * sizeof(HPackDesc), hipMemcpyHostToDevice, st));
        HIPCHK(h, hipStreamSynchronize(st));
        h->hpack_table_n = (int)h->hpack_jobs.size();
    }
    if (h->fwd_only[0]) {                                  // yn_train_forward: raw heads as dense fp32 rows, nothing else
        for (int k = 0; k < 3; ++k) launch_rows_to_f32(hd[k].out, 1, HCp, h->fwd_only[k], h->head_ch, hd[k].M, st);
        HIPCHK(h, hipGetLastError());
        return 0;
    }

    // =============================== loss (+ scaled gradient w.r.t. the raw heads) ===============================
    if (ensure_loss(h, B)) return 1;
    {
        GridInfo g = h->grid;
        g.head_ld = HCp;
        const h16* const heads[3] = {hd[0].out, hd[1].out, hd[2].out};
        h16* const gheads[3] = {hd[0].gout, hd[1].gout, hd[2].gout};
        const char* pe = getenv("YN_TRAIN_POISON");
        if (pe && atoi(pe)) HIPCHK(h, hipMemsetAsync(T.base + T.cap - T.gused, 0xff, T.gused, st));     // test hook: NaN-fill the gradient region first
        HIPCHK(h, hipMemsetAsync(gout_all, 0, gout_total * sizeof(h16), st));
        launch_loss_h16(heads, gheads, target_dev, g, B, h->loss_partial, losses_dev, h->scale_state, st);
    }

    // =============================== backward ===============================
    auto head_bwd = [&](int k, hipStream_t on, hipEvent_t e_done) {
        if (on) { T.flush_params(); T.st = on; }                                           // (queued weight gradients belong to the stream they were queued on)
        T.back(hd[k].r[4], hd[k].gout, HCp, 0, nullptr, vfull(hd[k].t[3], true), false, true, hd[k].r[3]);
        for (int j = 3; j >= 1; --j) T.back_dense(hd[k].r[j], hd[k].t[j], vfull(hd[k].t[j - 1], true), false, true, hd[k].r[j - 1]);
        T.back_dense(hd[k].r[0], hd[k].t[0], vfull(feats[k], true), false);               // first writer of p3a / p4b / p5a
        if (on) { T.flush_params(); (void)hipEventRecord(e_done, on); T.st = st; }
    };
    if (fk[0]) {
        (void)hipEventRecord(fev[4], st);                                                  // the loss is done: the towers' backward passes fork
        (void)hipStreamWaitEvent(fk[0], fev[4], 0); (void)hipStreamWaitEvent(fk[1], fev[4], 0);
    }
    head_bwd(0, fk[0], fev[5]);
    head_bwd(1, fk[1], fev[6]);
    head_bwd(2, nullptr, nullptr);                                                         // level 5 on the main stream: the neck's backward needs it first
    T.back_dense(r_sm3, p5a, vfull(d5, true), false);                                      // d5.g IS p5.g (d5 = p5 + down(p4b))
    if (fk[1]) (void)hipStreamWaitEvent(st, fev[6], 0);                                    // level 4's tower has written p4b.g
    launch_hresample(d5.g, nullptr, p4b.g, B, W5, W5, NECK, 3, st);
    T.back_dense(r_sm2, p4b, vfull(d4, true), false);
    if (fk[0]) (void)hipStreamWaitEvent(st, fev[5], 0);                                    // level 3's tower has written p3a.g
    launch_hresample(d4.g, nullptr, p3a.g, B, W4, W4, NECK, 3, st);
    T.back_dense(r_sm1, p3a, vfull(u3, true), false);
    launch_hresample(u3.g, nullptr, p4a.g, B, W3, W3, NECK, 2, st);
    T.back_dense(r_sm0, p4a, vfull(u4, true), false);
    launch_hresample(u4.g, nullptr, p5.g, B, W4, W4, NECK, 2, st);
    T.back_dense(r_lat2, p5, vfull(cfeat[2], true), false);                                // laterals: first writers of the stage outputs' gradients
    T.back_dense(r_lat1, p4, vfull(cfeat[1], true), false);
    T.back_dense(r_lat0, p3, vfull(cfeat[0], true), false);
    for (int bi = (int)blks.size() - 1; bi >= 0; --bi) {
        Blk& k = blks[bi];
        const int bf = k.bf;
        const long Mo = (long)B * k.Hout * k.Hout;
        if (!k.s2) {
            // in.g plane 0 <- even logical channels of out.g (the pass-through), plane 1 <- pw1's input gradient: written once each
            T.even_dst = k.in.g; T.even_ld = k.in.Cp; T.even_done = false;               // hbn_bwd_kernel writes the pass-through half on its way (it loads those values anyway)
            T.back(k.r_pw2, nullptr, 0, 0, &k.out, vfull(k.t2, true), false, true, k.r_dw);
            T.even_dst = nullptr;
            if (!T.even_done) launch_hgather(k.out.g, k.out.Cp, 0, 2, k.out.half, k.out.gap, k.in.g, k.in.Cp, 0, 1, k.in.half, 0, Mo, bf, k.in.half + k.in.gap, st);
            T.back_dense(k.r_dw, k.t2, vfull(k.t1, true), false, true, k.r_pw1);
            T.back_dense(k.r_pw1, k.t1, vplane(k.in, 1, true), false);
        } else {
            T.even_dst = k.tb1.g; T.even_ld = k.tb1.Cp; T.even_done = false;             // gradient of branch1's output = the even channels
            T.back(k.r_pw2, nullptr, 0, 0, &k.out, vfull(k.t2, true), false, true, k.r_dw);
            T.even_dst = nullptr;
            const bool b1_done = T.even_done;
            T.back_dense(k.r_dw, k.t2, vfull(k.t1, true), false, true, k.r_pw1);
            T.back_dense(k.r_pw1, k.t1, vfull(k.in, true), k.in.g != a1.g);                // previous stage's output: its lateral wrote first; the pool output: nobody did
            if (!b1_done) launch_hgather(k.out.g, k.out.Cp, 0, 2, k.out.half, k.out.gap, k.tb1.g, k.tb1.Cp, 0, 1, k.tb1.C, 0, Mo, bf, k.tb1.Cp, st);
            T.back_dense(k.r_b1pw, k.tb1, vfull(k.tdw1, true), false, true, k.r_b1dw);
            T.back_dense(k.r_b1dw, k.tdw1, vfull(k.in, true), true);
        }
    }
    if (stem_fuse) T.back_stem(r_stem, a1.g, pool_idx, B, H1);
    else {
        launch_hmaxpool_bwd(a1.g, pool_idx, B, H1, H1, 24, a0.g, st);
        T.back_dense(r_stem, a0, HV{}, false, false);
    }
    T.flush_params();
    if (T.side) {
        hipEvent_t e = h->train_events[HTrainer::NEV];
        HIPCHK(h, hipEventRecord(e, T.side));
        HIPCHK(h, hipStreamWaitEvent(st, e, 0));
    }
    launch_hgrad_finish(h->tG, T.gslots, (long)h->tN, (size_t)h->tN, h->scale_state, st);   // combine the slots, remove the loss scale, adapt it
    HIPCHK(h, hipGetLastError());
    return 0;
}

int train_step_h16(yn_handle* h, const float* x_dev, const float* target_dev, int B, float lr, float momentum, float weight_decay,
                   float grad_scale, int do_update, float* losses_dev)
{
    const int S = h->grid.S;
    hipStream_t st = h->stream;
    h->cur = st;
    // ---- host-side preparation: everything that allocates or synchronises ----
    const size_t need = network_arena_bytes(h, B, S) * 7 + ((size_t)256 << 20);       // fp16 tensors, padded channels; + the fixed fp32 scratch
    if (need > h->train_arena_bytes) {
        HIPCHK(h, hipStreamSynchronize(st));
        drop_train_graphs(h);
        if (h->train_arena) HIPCHK(h, hipFree(h->train_arena));
        HIPCHK(h, hipMalloc((void**)&h->train_arena, need));
        h->train_arena_bytes = need;
    }
    if (h->hpacks.empty()) h->hpacks.resize(h->layers.size());
    if (!h->scale_state) {
        HIPCHK(h, hipMalloc((void**)&h->scale_state, 8 * sizeof(float)));
        const char* e = getenv("YN_LOSS_SCALE");
        const float s0 = h->loss_scale_init >= 1.0f ? h->loss_scale_init : (e && atof(e) >= 1.0 ? (float)atof(e) : 1024.0f);
        const float init[8] = {s0, 1.0f / s0, h->loss_scale_clean, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        HIPCHK(h, hipMemcpyAsync(h->scale_state, init, sizeof init, hipMemcpyHostToDevice, st));
        HIPCHK(h, hipStreamSynchronize(st));
    }
    if (h->multi_stream && !h->profiling) {
        if (!h->train_side) {
            int least = 0, greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
            if (hipStreamCreateWithPriority(&h->train_side, hipStreamNonBlocking, least) != hipSuccess) h->train_side = nullptr;
        }
        for (int i = 0; i < 2; ++i)
            if (!h->train_fork[i] && hipStreamCreateWithFlags(&h->train_fork[i], hipStreamNonBlocking) != hipSuccess) h->train_fork[i] = nullptr;
        while (h->train_side && h->train_events.size() < (size_t)HTrainer::NEV + 9) {
            hipEvent_t e;
            HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
            h->train_events.push_back(e);
        }
    }
    if (ensure_loss(h, B)) return 1;
    if (!h->train_losses) HIPCHK(h, hipMalloc((void**)&h->train_losses, 4 * sizeof(float)));

    // ---- the body: direct, or replayed from / captured into a hipGraph ----
    // Opt-in (yn_train_graph): measured at 608 / bs 32 the replayed step takes 8.93 ms against 8.50 ms for direct launches -
    // the runtime serialises more of the two-stream graph than the streams themselves do, and the direct path's remaining queue gaps are
    // only ~0.35 ms.  The graph is keyed by everything the launches bake in (x and target pointers, B, S, the executor's switches; the
    // losses go through a buffer of the handle); the first two steps of a key run directly (they allocate: weight packs, the pack table),
    // the four most recent keys are kept, and a caller whose tensors' addresses never repeat stays on direct launches.
    // Head-tower forks: worth 0.25 ms when the three streams land on hardware queues of their own, but measured at 13.1 ms against 8.5 ms in a
    // process that already holds many streams (the default bench.py run, after the inference rigs: the runtime multiplexes streams onto a few
    // hardware queues and the forks then serialise behind each other).  So the handle decides by measurement: steps 3-6 of its life run
    // alternately with and without the forks between two timing events, the faster form (minimum of its two samples) stays.
    int trial = -1;
    if (h->head_fork >= 0) h->head_fork_now = h->head_fork;
    else if (!h->hpack_table || h->fwd_only[0] || !h->train_fork[0] || !h->train_fork[1] || !h->train_side) h->head_fork_now = 0;       // not yet (steps 1-2 allocate)
    else if (h->fork_trials < 4) {
        trial = h->fork_trials++;
        for (int i = 0; i < 8; ++i)
            if (!h->fork_ev[i]) HIPCHK(h, hipEventCreate(&h->fork_ev[i]));
        h->head_fork_now = (trial & 1) == 0;
        HIPCHK(h, hipEventRecord(h->fork_ev[2 * trial], st));
    } else {
        HIPCHK(h, hipEventSynchronize(h->fork_ev[7]));
        float ms[4] = {0, 0, 0, 0};
        for (int i = 0; i < 4; ++i) (void)hipEventElapsedTime(&ms[i], h->fork_ev[2 * i], h->fork_ev[2 * i + 1]);
        const float with_forks = ms[0] < ms[2] ? ms[0] : ms[2], without = ms[1] < ms[3] ? ms[1] : ms[3];
        h->head_fork = with_forks < 0.98f * without ? 1 : 0;
        h->head_fork_now = h->head_fork;
    }
    const bool graphable = h->train_graph && st != nullptr && !h->profiling && !h->fwd_only[0] && !getenv("YN_TRAIN_POISON") && h->train_graph_misses < 64;
    int rc = 0;
    bool ran = false;
    if (graphable) {
        // the per-step test switches select different launches (and a different arena carve): part of the key, or a flipped switch replays the stale form
        auto sw = [](const char* v) { return (uintptr_t)(v ? atoi(v) + 1 : 0); };
        const std::vector<uintptr_t> key{(uintptr_t)x_dev, (uintptr_t)target_dev, (uintptr_t)B, (uintptr_t)S, (uintptr_t)h->multi_stream, (uintptr_t)h->head_fork_now,
                                         sw(getenv("YN_TRAIN_FUSE_STATS")) | sw(getenv("YN_TRAIN_FUSE_SUMS")) << 8 | sw(getenv("YN_TRAIN_STEM_FUSE")) << 16};
        TrainGraph* tg = nullptr;
        for (TrainGraph& g : h->train_graphs) if (g.key == key) { tg = &g; break; }
        if (!tg) {
            ++h->train_graph_misses;
            if (h->train_graphs.size() >= 4) {                         // keep the four most recent keys
                HIPCHK(h, hipStreamSynchronize(st));
                if (h->train_graphs.front().exec) (void)hipGraphExecDestroy(h->train_graphs.front().exec);
                h->train_graphs.erase(h->train_graphs.begin());
            }
            h->train_graphs.push_back(TrainGraph{key, nullptr, 0});
            tg = &h->train_graphs.back();
        } else if (h->train_graph_misses > 0) --h->train_graph_misses;
        if (tg->exec && trial < 0) { HIPCHK(h, hipGraphLaunch(tg->exec, st)); ran = true; ++h->train_graph_replays; }
        else if (tg->direct_runs >= 2 && h->hpack_table && trial < 0 && !tg->exec) {
            hipGraph_t graph = nullptr;
            HIPCHK(h, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
            rc = train_body_h16(h, x_dev, target_dev, B, h->train_losses);
            const hipError_t e = hipStreamEndCapture(st, &graph);
            if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
            if (e != hipSuccess) return fail(h, "hipStreamEndCapture (training step) failed: %s", hipGetErrorString(e));
            HIPCHK(h, hipGraphInstantiate(&tg->exec, graph, nullptr, nullptr, 0));
            (void)hipGraphDestroy(graph);
            HIPCHK(h, hipGraphLaunch(tg->exec, st));
            ran = true; ++h->train_graph_replays;
        } else ++tg->direct_runs;
    }
    if (!ran) {
        rc = train_body_h16(h, x_dev, target_dev, B, h->train_losses);
        if (rc) return rc;
    }
    if (trial >= 0) HIPCHK(h, hipEventRecord(h->fork_ev[2 * trial + 1], st));
    if (h->fwd_only[0]) return 0;
    if (losses_dev) HIPCHK(h, hipMemcpyAsync(losses_dev, h->train_losses, 4 * sizeof(float), hipMemcpyDeviceToDevice, st));

    if (do_update) {
        if (!h->skip_flag) {
            HIPCHK(h, hipMalloc((void**)&h->skip_flag, 2 * sizeof(int)));
            HIPCHK(h, hipMemsetAsync(h->skip_flag, 0, 2 * sizeof(int), st));
        }
        launch_sgd(h->tP, h->tG, h->tM, (long)h->tN, lr, momentum, weight_decay, grad_scale, 0, h->skip_flag, st);
        launch_hscale_update(h->scale_state, h->skip_flag, st);
        h->train_steps++;
        HIPCHK(h, hipGetLastError());
    }
    h->folded = false;
    return 0;
}

}  // namespace
