// yn_train.inc — the training step (SURVEY §8 row 20), included by yn_api.hip.
//
// train.py:219-231 — `model(images, target)` in train mode (BatchNorm batch statistics), the four losses,
// `total_loss.backward()`, `optimizer.step()` — restated as an explicit forward tape + hand-written backward over the
// kernels of kernels_conv.hip / kernels_bwd.hip / kernels_train.hip.  Parameters, gradients and momentum live in three
// caller-owned FLAT float32 buffers (order = nn.Module.named_parameters() of the reference model), so the gradient
// exchange of data-parallel training is ONE all-reduce over `grads` between yn_train_step(do_update = 0) and yn_sgd_step.
//
// Correctness-first: fp32 throughout, no buffer reuse, weight packs rebuilt every step.

namespace {

struct View { float* p; int ld, off, cs; };             // channel c of row m: p[m*ld + off + c*cs]

struct TRec {                                           // one conv (+BN +act) executed in train mode
    const Layer* l = nullptr;
    View x{};                                           // conv input (cs = 1)
    int B = 0, H = 0, W = 0;                            // input spatial extent
    long Mi = 0, Mo = 0;
    float* y = nullptr; int y_ld = 0;                   // conv output, pre-BN (the layer output itself when there is no BN)
    View z{};                                           // BN+act output view
    float *mean = nullptr, *invstd = nullptr;
    double* acc = nullptr;                              // [4][C] zeroed at step start: forward sums, backward sums
    const float* x_nchw = nullptr;                      // stem
};

struct Trainer {
    yn_handle* h;
    int B, S;
    hipStream_t st;
    char* base; size_t used = 0, cap;
    size_t gused = 0;                                   // gradient tensors grow down from the end of the arena: ONE memset zeroes them all
    std::vector<TRec> recs;
    float* tmp = nullptr;
    // Weight gradients run on a side stream, concurrently with the BN-backward / input-gradient chain on the main stream:
    // they only depend on dy (and the saved activations) and nothing but the optimiser waits for them.  The BatchNorm backward
    // writes dy IN PLACE over the pre-BN conv output (nothing reads y afterwards), so no buffer is reused and the side stream only
    // waits for the main one: one event per BATCH layers (round 3, as in the fp16 executor: an event record costs the main queue
    // ~7 us of idle time, and there were 150 per step).
    static constexpr int NEV = 32, BATCH = 4;
    hipStream_t side = nullptr;
    hipEvent_t ev[NEV];
    int ei = 0;
    struct Pending { const TRec* r; const float* d; int ld; };
    std::vector<Pending> pending;
    double* stats = nullptr; size_t stats_used = 0, stats_cap = 0;     // BatchNorm sum accumulators, one memset per step
    float* wpart = nullptr; size_t wpart_cap = 0;                        // per-slice weight-gradient copies of one layer at a time
    float* gslots = nullptr;                                            // GRAD_SLOTS copies of the flat gradient buffer (atomics targets)
    bool oom = false;

    float* take(size_t floats)
    {
        const size_t bytes = (floats * sizeof(float) + 255) & ~(size_t)255;
        if (used + bytes + gused > cap) { oom = true; return (float*)base; }
        float* p = (float*)(base + used);
        used += bytes;
        return p;
    }
    float* take_g(size_t floats)
    {
        const size_t bytes = (floats * sizeof(float) + 255) & ~(size_t)255;
        if (used + bytes + gused > cap) { oom = true; return (float*)base; }
        gused += bytes;
        return (float*)(base + cap - gused);
    }
    float* P(const std::string& k) { return h->tP + h->toff.at(k); }
    float* G(const std::string& k) { return h->tG + h->toff.at(k); }
    float* GS(const std::string& k) { return gslots + h->toff.at(k); }   // slot 0; slot s is h->tN floats further
    const TrainPack& pack(const Layer& l) { return h->tpacks[(size_t)(&l - &h->layers[0])]; }

    // ---- forward pieces ----
    TRec& conv(const Layer& l, View x, int B_, int H, int W, const float* x_nchw = nullptr)
    {
        TRec r;
        r.l = &l; r.x = x; r.B = B_; r.H = H; r.W = W; r.x_nchw = x_nchw;
        const int Ho = (H - 1) / l.stride + 1, Wo = (W - 1) / l.stride + 1;
        r.Mi = (long)B_ * H * W; r.Mo = (long)B_ * Ho * Wo;
        r.y_ld = l.cout;
        r.y = take((size_t)r.Mo * r.y_ld);
        const TrainPack& pk = pack(l);
        if (l.kind == K_PW) {
            GemmArgs a{};
            a.in = x.p; a.in_ld = x.ld; a.in_off = x.off; a.Wp = pk.wp; a.bias = pk.bias;
            a.out = r.y; a.out_ld = r.y_ld; a.M = (int)r.Mo; a.K = l.cin; a.N = l.cout; a.Npad = l.Npad; a.act = 0; a.cfg = tune_pw(h, a);      // per-shape tile choice, timed once (as in inference)
            launch_pw(a, st);
        } else if (l.kind == K_DW) {
            DwArgs a{};
            a.in = x.p; a.in_ld = x.ld; a.in_off = x.off; a.w = pk.wp; a.bias = pk.bias; a.out = r.y; a.out_ld = r.y_ld; a.out_off = 0;
            a.B = B_; a.H = H; a.W = W; a.C = l.cout; a.stride = l.stride; a.act = 0;
            launch_dw(a, st);
        } else if (l.kind == K_DENSE3) {
            GemmArgs a{};
            a.in = x.p; a.in_ld = x.ld; a.in_off = x.off; a.resample = 0; a.H = H; a.W = W; a.Wp = pk.wp; a.bias = pk.bias;
            a.out = r.y; a.out_ld = r.y_ld; a.M = (int)r.Mo; a.K = l.cin; a.N = l.cout; a.Npad = l.Npad; a.act = 0; a.cfg = -1;
            launch_conv3x3(a, st);
        } else {
            launch_stem(x_nchw, B_, H, W, pk.wp, pk.bias, l.cout, 0, r.y, st);
        }
        recs.push_back(r);
        return recs.back();
    }
    // BatchNorm (batch statistics) + activation into `out`; optional concat+shuffle pass-through
    void bn(TRec& r, View out, const float* pass = nullptr, int pass_ld = 0, int pass_off = 0, int pass_dst_off = 0)
    {
        const Layer& l = *r.l;
        r.mean = take(l.cout); r.invstd = take(l.cout);
        if (stats_used + 4 * ACC_SLOTS * (size_t)l.cout > stats_cap) { oom = true; return; }
        r.acc = stats + stats_used; stats_used += 4 * ACC_SLOTS * (size_t)l.cout;
        launch_bn_stats(r.y, (int)r.Mo, l.cout, r.acc, st);
        BnApplyArgs a{};
        a.y = r.y; a.acc = r.acc; a.eps = 1e-5f; a.mean = r.mean; a.invstd = r.invstd; a.gamma = P(l.bn + ".weight"); a.beta = P(l.bn + ".bias");
        a.out = out.p; a.out_ld = out.ld; a.out_off = out.off; a.out_cs = out.cs;
        a.pass = pass; a.pass_ld = pass_ld; a.pass_off = pass_off; a.pass_dst_off = pass_dst_off;
        const Param* rm = find_param(h, l.bn + ".running_mean");
        const Param* rv = find_param(h, l.bn + ".running_var");
        a.rmean = rm ? (float*)rm->dev : nullptr; a.rvar = rv ? (float*)rv->dev : nullptr; a.momentum = 0.1f;
        a.M = (int)r.Mo; a.C = l.cout; a.act = l.act;
        launch_bn_apply(a, st);
        r.z = out;
    }

    // ---- backward pieces ----
    // gradient w.r.t. the conv output (through act + BN), parameter gradients of BN / bias / weights. Returns (dy, ld).
    const float* back_params(const TRec& r, View dz, int* dy_ld)
    {
        const Layer& l = *r.l;
        const float* d;
        if (!l.bn.empty()) {
            BnBwdArgs a{};
            a.dz = dz.p; a.dz_ld = dz.ld; a.dz_off = dz.off; a.dz_cs = dz.cs;
            float* dy = r.y;                                      // in place
            a.y = r.y; a.mean = r.mean; a.invstd = r.invstd; a.gamma = P(l.bn + ".weight"); a.beta = P(l.bn + ".bias"); a.dy = dy; a.M = (int)r.Mo; a.C = l.cout; a.act = l.act;
            a.acc = r.acc + 2 * ACC_SLOTS * (size_t)l.cout; a.dgamma = G(l.bn + ".weight"); a.dbeta = G(l.bn + ".bias");
            launch_bn_bwd(a, st);
            d = dy; *dy_ld = l.cout;
        } else {
            d = dz.p + dz.off; *dy_ld = dz.ld;            // plain conv output (head): dz is dense, cs = 1
        }
        if (!side) { params_on_side(r, d, *dy_ld); return d; }
        pending.push_back(Pending{&r, d, *dy_ld});
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
        for (const Pending& p : pending) params_on_side(*p.r, p.d, p.ld);
        pending.clear();
    }
    // bias / weight gradients of one layer from dy, on the side stream when there is one
    void params_on_side(const TRec& r, const float* d, int d_ld)
    {
        const Layer& l = *r.l;
        hipStream_t st = side ? side : this->st;
        int ld_v = d_ld; int* dy_ld = &ld_v;
        // a conv bias in front of a train-mode BatchNorm has an exactly zero gradient (the batch mean removes it): its
        // slice of the zeroed gradient buffer is left alone; torch computes round-off noise of ~1e-7 * |dy| there.
        if (l.has_bias && l.bn.empty()) launch_col_sum_accumulate(d, *dy_ld, 0, (int)r.Mo, l.cout, GS(l.conv + ".bias"), (size_t)h->tN, st);
        if (l.kind == K_PW || l.kind == K_DENSE3) {
            WgradArgs a{};
            a.dy = d; a.dy_ld = *dy_ld; a.x = r.x.p; a.x_ld = r.x.ld; a.x_off = r.x.off; a.H = r.H; a.W = r.W; a.Cin = l.cin;
            a.dense = l.kind == K_DENSE3; a.dw = G(l.conv + ".weight"); a.partial = wpart; a.partial_cap = wpart_cap; a.M = (int)r.Mo; a.N = l.cout; a.K = a.dense ? 9 * l.cin : l.cin;
            launch_wgrad(a, st);
        } else if (l.kind == K_DW) {
            launch_dw_wgrad(d, r.x.p, r.x.ld, r.x.off, r.B, r.H, r.W, l.cout, l.stride, GS(l.conv + ".weight"), wpart, wpart_cap, st);
        } else {
            launch_stem_wgrad(d, r.x_nchw, r.B, r.H, r.W, l.cout, G(l.conv + ".weight"), wpart, wpart_cap, st);
        }
    }
    // gradient w.r.t. the conv input, written (or accumulated) into dx (cs = 1)
    void back_input(const TRec& r, const float* d, int d_ld, View dx, bool accumulate)
    {
        const Layer& l = *r.l;
        const TrainPack& pk = pack(l);
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
    // whole layer backward: dz (gradient of the layer's output view) -> parameter grads + input gradient
    void back(int ri, View dz, View dx, bool accumulate, bool need_input = true)
    {
        int ld = 0;
        const float* d = back_params(recs[ri], dz, &ld);
        if (need_input) back_input(recs[ri], d, ld, dx, accumulate);
    }
};

int train_bind_layers(yn_handle* h)
{
    // flat order == named_parameters(): conv.weight, [conv.bias], [bn.weight, bn.bias] per layer, layers in module order
    h->toff.clear();
    size_t off = 0;
    for (const Layer& l : h->layers) {
        const size_t wn = l.kind == K_DW ? (size_t)l.cout * 9 : (l.kind == K_PW ? (size_t)l.cout * l.cin : (size_t)l.cout * l.cin * 9);
        h->toff[l.conv + ".weight"] = off; off += wn;
        if (l.has_bias) { h->toff[l.conv + ".bias"] = off; off += l.cout; }
        if (!l.bn.empty()) { h->toff[l.bn + ".weight"] = off; off += l.cout; h->toff[l.bn + ".bias"] = off; off += l.cout; }
    }
    h->tN_expected = (int64_t)off;
    return 0;
}

}  // namespace

#include "yn_train_h16.inc"

#pragma GCC visibility push(default)
extern "C" {

int64_t yn_train_param_count(yn_handle* h)
{
    if (!h) return -1;
    if (h->toff.empty()) train_bind_layers(h);
    return h->tN_expected;
}

int yn_train_param_offset(yn_handle* h, const char* key, int64_t* offset, int64_t* numel)
{
    YN_ENTER(h);
    if (h->toff.empty()) train_bind_layers(h);
    auto it = h->toff.find(key);
    if (it == h->toff.end()) return fail(h, "'%s' is not a trainable parameter", key);
    const Param* p = find_param(h, key);
    if (offset) *offset = (int64_t)it->second;
    if (numel) *numel = p ? (int64_t)p->numel : -1;
    return 0;
}

int yn_train_bind(yn_handle* h, float* params, float* grads, float* momentum, int64_t n)
{
    YN_ENTER(h);
    train_bind_layers(h);
    if (n != h->tN_expected) return fail(h, "yn_train_bind: flat buffers hold %lld floats, the model has %lld trainable elements", (long long)n, (long long)h->tN_expected);
    if (!params || !grads || !momentum) return fail(h, "yn_train_bind: null buffer");
    drop_train_graphs(h);                                   // captured steps bake the flat buffers' addresses in
    // seed the flat parameter buffer from the loaded state dict
    for (const auto& kv : h->toff) {
        const Param* p = find_param(h, kv.first);
        if (!p) return fail(h, "yn_train_bind: parameter '%s' was never loaded", kv.first.c_str());
        HIPCHK(h, hipMemcpyAsync(params + kv.second, p->dev, p->numel * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    }
    for (const Layer& l : h->layers)
        if (!l.bn.empty() && (!find_param(h, l.bn + ".running_mean") || !find_param(h, l.bn + ".running_var")))
            return fail(h, "yn_train_bind: BatchNorm statistics of '%s' were never loaded (a fused model cannot be trained)", l.bn.c_str());
    HIPCHK(h, hipMemsetAsync(grads, 0, n * sizeof(float), h->stream));
    HIPCHK(h, hipMemsetAsync(momentum, 0, n * sizeof(float), h->stream));
    h->tP = params; h->tG = grads; h->tM = momentum; h->tN = n; h->train_steps = 0;
    if (h->hpack_table) { HIPCHK(h, hipStreamSynchronize(h->stream)); (void)hipFree(h->hpack_table); h->hpack_table = nullptr; h->hpack_table_n = 0; }
    h->hpack_jobs.clear();                                 // the fp16 step's pack table points into the (new) flat parameter buffer
    if (!h->zeros) {
        HIPCHK(h, hipMalloc((void**)&h->zeros, 4096 * sizeof(float)));
        HIPCHK(h, hipMemsetAsync(h->zeros, 0, 4096 * sizeof(float), h->stream));
    }
    // per-layer packs (forward: raw weights; backward: transposed / flipped)
    if (h->tpacks.empty()) {
        h->tpacks.resize(h->layers.size());
        for (size_t i = 0; i < h->layers.size(); ++i) {
            Layer& l = h->layers[i];
            TrainPack& pk = h->tpacks[i];
            size_t fwd, bwd;
            int Kp, Npad;
            if (l.kind == K_DW) { fwd = (size_t)9 * l.cout; bwd = fwd; Kp = 9; Npad = l.cout; }
            else if (l.kind == K_STEM) { fwd = (size_t)27 * l.cout; bwd = 0; Kp = 27; Npad = l.cout; }
            else {
                const int K = l.cin * (l.kind == K_DENSE3 ? 9 : 1);
                Kp = (K + 1) & ~1; Npad = (l.cout + 31) & ~31; fwd = (size_t)Kp * Npad;
                const int Kb = l.cout * (l.kind == K_DENSE3 ? 9 : 1);
                pk.Kb = (Kb + 1) & ~1; pk.Npad_b = (l.cin + 31) & ~31; bwd = (size_t)pk.Kb * pk.Npad_b;
                if (l.kind == K_DENSE3) pk.Kb = l.cout;              // conv3x3 launcher takes Cin', not 9*Cin'
            }
            l.Kp = Kp; l.Npad = Npad;                                // the same values yn_fold_bn derives
            HIPCHK(h, hipMalloc((void**)&pk.wp, fwd * sizeof(float)));
            HIPCHK(h, hipMalloc((void**)&pk.bias, (size_t)((Npad + 31) & ~31) * sizeof(float)));
            HIPCHK(h, hipMemsetAsync(pk.wp, 0, fwd * sizeof(float), h->stream));
            HIPCHK(h, hipMemsetAsync(pk.bias, 0, (size_t)((Npad + 31) & ~31) * sizeof(float), h->stream));
            if (bwd) {
                HIPCHK(h, hipMalloc((void**)&pk.wp_bwd, bwd * sizeof(float)));
                HIPCHK(h, hipMemsetAsync(pk.wp_bwd, 0, bwd * sizeof(float), h->stream));
            }
        }
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int yn_train_step(yn_handle* h, const float* x_dev, const float* target_dev, int B, float lr, float momentum, float weight_decay,
                  float grad_scale, int do_update, float* losses_dev)
{
    YN_ENTER(h);
    if (!h->tP) return fail(h, "yn_train_step before yn_train_bind");
    if (B <= 0) return fail(h, "batch must be positive (got %d)", B);
    if (h->train_dtype == YN_F16) return train_step_h16(h, x_dev, target_dev, B, lr, momentum, weight_decay, grad_scale, do_update, losses_dev);
    const int S = h->grid.S;
    hipStream_t st = h->stream;
    h->cur = st;
    // ---- workspace ----
    const size_t need = network_arena_bytes(h, B, S) * 10 + ((size_t)256 << 20);      // activations + gradients, plus the fixed scratch (weight-gradient slices, gradient slots, BN sums)
    if (need > h->train_arena_bytes) {
        HIPCHK(h, hipStreamSynchronize(st));
        if (h->train_arena) HIPCHK(h, hipFree(h->train_arena));
        HIPCHK(h, hipMalloc((void**)&h->train_arena, need));
        h->train_arena_bytes = need;
    }
    Trainer T{h, B, S, st, h->train_arena, 0, h->train_arena_bytes};
    T.recs.reserve(h->layers.size() + 4);
    const long Mmax = (long)B * (S / 2) * (S / 2);
    const int HCp = (h->head_ch + 3) & ~3;
    {
        // the largest dy / accumulate-scratch of any layer: the stem's 24 channels at S/2, or a padded head row at S/8
        const size_t dyn = (size_t)Mmax * 24 > (size_t)B * (S / 8) * (S / 8) * HCp ? (size_t)Mmax * 24 : (size_t)B * (S / 8) * (S / 8) * HCp;
        T.tmp = T.take(dyn);
    }
    if (h->multi_stream && !h->profiling) {
        if (!h->side[0] && hipStreamCreateWithFlags(&h->side[0], hipStreamNonBlocking) != hipSuccess) h->side[0] = nullptr;
        if (h->side[0]) {
            while (h->train_events.size() < (size_t)Trainer::NEV + 1) {
                hipEvent_t e;
                HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
                h->train_events.push_back(e);
            }
            T.side = h->side[0];
            for (int i = 0; i < Trainer::NEV; ++i) T.ev[i] = h->train_events[i];
        }
    }
    {
        size_t nstat = 0;
        for (const Layer& l : h->layers) if (!l.bn.empty()) nstat += 4 * ACC_SLOTS * (size_t)l.cout;
        T.stats = (double*)T.take(nstat * 2);
        T.stats_cap = nstat;
        HIPCHK(h, hipMemsetAsync(T.stats, 0, nstat * sizeof(double), st));
        T.wpart_cap = (size_t)16 << 20;
        T.wpart = T.take(T.wpart_cap);
        T.gslots = T.take((size_t)GRAD_SLOTS * h->tN);
        HIPCHK(h, hipMemsetAsync(T.gslots, 0, (size_t)GRAD_SLOTS * h->tN * sizeof(float), st));
    }

    // ---- gradients start at zero; weight packs follow the current parameters ----
    HIPCHK(h, hipMemsetAsync(h->tG, 0, h->tN * sizeof(float), st));
    for (size_t i = 0; i < h->layers.size(); ++i) {
        const Layer& l = h->layers[i];
        TrainPack& pk = h->tpacks[i];
        FoldArgs a{};
        a.w = T.P(l.conv + ".weight"); a.b = l.has_bias ? T.P(l.conv + ".bias") : nullptr; a.eps = 1e-5f; a.Cout = l.cout; a.Cin = l.cin;
        size_t fwd;
        if (l.kind == K_DW) { a.kind = 1; a.kk = 9; fwd = (size_t)9 * l.cout; a.Npad = l.cout; a.Kp = 9; }
        else if (l.kind == K_STEM) { a.kind = 2; a.kk = 9; fwd = (size_t)27 * l.cout; a.Npad = l.cout; a.Kp = 27; }
        else { a.kind = 0; a.kk = l.kind == K_DENSE3 ? 9 : 1; a.Kp = (l.cin * a.kk + 1) & ~1; a.Npad = (l.cout + 31) & ~31; fwd = (size_t)a.Kp * a.Npad; }
        (void)fwd;                                            // padding of the packs was zeroed once in yn_train_bind
        a.w_packed = pk.wp; a.b_packed = pk.bias;
        launch_fold_pack(a, st);
        if (pk.wp_bwd) {
            if (l.kind == K_DW) launch_pack_bwd(a.w, l.cout, 1, 1, 0, pk.wp_bwd, st);
            else {
                launch_pack_bwd(a.w, l.cout, l.cin, l.kind == K_DENSE3 ? 2 : 0, pk.Npad_b, pk.wp_bwd, st);
            }
        }
    }

    // =============================== forward (train mode) ===============================
    auto dense = [&](float* p, int C) { return View{p, C, 0, 1}; };
    struct TT { float* v; float* g; long M; int C; };
    auto mk = [&](long M, int C) { TT t{T.take((size_t)M * C), T.take_g((size_t)M * C), M, C}; return t; };

    const int H1 = S / 2, H2 = S / 4;
    const long M1 = (long)B * H1 * H1, M2 = (long)B * H2 * H2;
    TT a0 = mk(M1, 24), a1 = mk(M2, 24);
    int32_t* pool_idx = (int32_t*)T.take((size_t)M2 * 24);
    const int r_stem = (int)T.recs.size();
    { TRec& r = T.conv(L(h, "stem"), View{nullptr, 0, 0, 1}, B, S, S, x_dev); T.bn(r, dense(a0.v, 24)); }
    launch_maxpool_idx(a0.v, B, H1, H1, 24, a1.v, pool_idx, st);

    struct Blk { int s2; int r_b1dw, r_b1pw, r_pw1, r_dw, r_pw2; TT in, tdw1, tb1, t1, t2, out; int Hin, Hout, Cin, C, bf; };
    std::vector<Blk> blks;
    TT cur = a1;
    int curC = 24, curH = H2;
    TT cfeat[3];
    char nm[96];
    for (int si = 0; si < 3; ++si) {
        const int C = h->stage_ch[si], bf = C / 2;
        for (int bi = 0; bi < STAGE_REP[si]; ++bi) {
            snprintf(nm, sizeof nm, "backbone.stage%d.%d", si + 2, bi);
            const std::string Pn = nm;
            Blk k{};
            k.in = cur; k.Cin = curC; k.C = C; k.bf = bf; k.Hin = curH;
            if (bi == 0) {
                const int Ho = curH / 2;
                const long Mi = (long)B * curH * curH, Mo = (long)B * Ho * Ho;
                k.s2 = 1; k.Hout = Ho;
                k.tdw1 = mk(Mo, curC); k.tb1 = mk(Mo, bf); k.t1 = mk(Mi, bf); k.t2 = mk(Mo, bf); k.out = mk(Mo, C);
                k.r_b1dw = (int)T.recs.size(); { TRec& r = T.conv(L(h, Pn + ".b1.dw"), dense(cur.v, curC), B, curH, curH); T.bn(r, dense(k.tdw1.v, curC)); }
                k.r_b1pw = (int)T.recs.size(); { TRec& r = T.conv(L(h, Pn + ".b1.pw"), dense(k.tdw1.v, curC), B, Ho, Ho); T.bn(r, dense(k.tb1.v, bf)); }
                k.r_pw1 = (int)T.recs.size(); { TRec& r = T.conv(L(h, Pn + ".b2.pw1"), dense(cur.v, curC), B, curH, curH); T.bn(r, dense(k.t1.v, bf)); }
                k.r_dw = (int)T.recs.size(); { TRec& r = T.conv(L(h, Pn + ".b2.dw"), dense(k.t1.v, bf), B, curH, curH); T.bn(r, dense(k.t2.v, bf)); }
                k.r_pw2 = (int)T.recs.size(); { TRec& r = T.conv(L(h, Pn + ".b2.pw2"), dense(k.t2.v, bf), B, Ho, Ho);
                                                 T.bn(r, View{k.out.v, C, 1, 2}, k.tb1.v, bf, 0, 0); }          // out[2j] = b1[j], out[2j+1] = b2[j]
                curH = Ho;
            } else {
                const long Mo = (long)B * curH * curH;
                k.s2 = 0; k.Hout = curH;
                k.t1 = mk(Mo, bf); k.t2 = mk(Mo, bf); k.out = mk(Mo, C);
                k.r_pw1 = (int)T.recs.size(); { TRec& r = T.conv(L(h, Pn + ".b2.pw1"), View{cur.v, C, bf, 1}, B, curH, curH); T.bn(r, dense(k.t1.v, bf)); }
                k.r_dw = (int)T.recs.size(); { TRec& r = T.conv(L(h, Pn + ".b2.dw"), dense(k.t1.v, bf), B, curH, curH); T.bn(r, dense(k.t2.v, bf)); }
                k.r_pw2 = (int)T.recs.size(); { TRec& r = T.conv(L(h, Pn + ".b2.pw2"), dense(k.t2.v, bf), B, curH, curH);
                                                 T.bn(r, View{k.out.v, C, 1, 2}, cur.v, C, 0, 0); }              // out[2j] = x1[j]
            }
            cur = k.out; curC = C;
            blks.push_back(k);
        }
        cfeat[si] = cur;
    }
    // neck
    const int W3 = S / 8, W4 = S / 16, W5 = S / 32;
    const long M3 = (long)B * W3 * W3, M4 = (long)B * W4 * W4, M5 = (long)B * W5 * W5;
    TT p3 = mk(M3, NECK), p4 = mk(M4, NECK), p5 = mk(M5, NECK);
    TT u4 = mk(M4, NECK), p4a = mk(M4, NECK), u3 = mk(M3, NECK), p3a = mk(M3, NECK), d4 = mk(M4, NECK), p4b = mk(M4, NECK), d5 = mk(M5, NECK), p5a = mk(M5, NECK);
    // u = p + up2(q) / d = p + down(q): the sum's gradient IS the gradient of its same-resolution term: one buffer (four device copies less)
    p5.g = d5.g; p4a.g = d4.g; p3.g = u3.g; p4.g = u4.g;
    const int r_lat0 = (int)T.recs.size(); { TRec& r = T.conv(L(h, "conv1x1_0"), dense(cfeat[0].v, h->stage_ch[0]), B, W3, W3); T.bn(r, dense(p3.v, NECK)); }
    const int r_lat1 = (int)T.recs.size(); { TRec& r = T.conv(L(h, "conv1x1_1"), dense(cfeat[1].v, h->stage_ch[1]), B, W4, W4); T.bn(r, dense(p4.v, NECK)); }
    const int r_lat2 = (int)T.recs.size(); { TRec& r = T.conv(L(h, "conv1x1_2"), dense(cfeat[2].v, h->stage_ch[2]), B, W5, W5); T.bn(r, dense(p5.v, NECK)); }
    launch_resample(p4.v, p5.v, u4.v, B, W4, W4, NECK, 0, st);
    const int r_sm0 = (int)T.recs.size(); { TRec& r = T.conv(L(h, "smooth_0"), dense(u4.v, NECK), B, W4, W4); T.bn(r, dense(p4a.v, NECK)); }
    launch_resample(p3.v, p4a.v, u3.v, B, W3, W3, NECK, 0, st);
    const int r_sm1 = (int)T.recs.size(); { TRec& r = T.conv(L(h, "smooth_1"), dense(u3.v, NECK), B, W3, W3); T.bn(r, dense(p3a.v, NECK)); }
    launch_resample(p4a.v, p3a.v, d4.v, B, W4, W4, NECK, 1, st);
    const int r_sm2 = (int)T.recs.size(); { TRec& r = T.conv(L(h, "smooth_2"), dense(d4.v, NECK), B, W4, W4); T.bn(r, dense(p4b.v, NECK)); }
    launch_resample(p5.v, p4b.v, d5.v, B, W5, W5, NECK, 1, st);
    const int r_sm3 = (int)T.recs.size(); { TRec& r = T.conv(L(h, "smooth_3"), dense(d5.v, NECK), B, W5, W5); T.bn(r, dense(p5a.v, NECK)); }
    // heads
    TT feats[3] = {p3a, p4b, p5a};
    const int Ws[3] = {W3, W4, W5};
    struct HeadT { TT t[4]; int r[5]; float* out; float* gout; long M; };
    HeadT hd[3];
    for (int k = 0; k < 3; ++k) {
        const long M = (long)B * Ws[k] * Ws[k];
        snprintf(nm, sizeof nm, "head_det_%d", k + 1);
        const std::string Pn = nm;
        hd[k].M = M;
        for (int j = 0; j < 4; ++j) hd[k].t[j] = mk(M, NECK);
        hd[k].out = T.take((size_t)M * HCp);
        hd[k].gout = T.take_g((size_t)M * HCp);
        const float* in = feats[k].v;
        for (int j = 0; j < 4; ++j) {
            hd[k].r[j] = (int)T.recs.size();
            TRec& r = T.conv(L(h, Pn + "." + std::to_string(j)), dense((float*)in, NECK), B, Ws[k], Ws[k]);
            T.bn(r, dense(hd[k].t[j].v, NECK));
            in = hd[k].t[j].v;
        }
        hd[k].r[4] = (int)T.recs.size();
        {   // final 1x1 conv with bias, written with the padded row stride HCp (extra column = 0)
            const Layer& l = L(h, Pn + ".4");
            TRec r;
            r.l = &l; r.x = dense((float*)in, NECK); r.B = B; r.H = Ws[k]; r.W = Ws[k]; r.Mi = r.Mo = M; r.y = hd[k].out; r.y_ld = HCp;
            r.z = View{hd[k].out, HCp, 0, 1};
            const TrainPack& pk = T.pack(l);
            GemmArgs a{};
            a.in = in; a.in_ld = NECK; a.Wp = pk.wp; a.bias = pk.bias; a.out = hd[k].out; a.out_ld = HCp; a.M = (int)M; a.K = NECK;
            a.N = HCp <= l.Npad ? HCp : l.cout; a.Npad = l.Npad; a.act = 0; a.cfg = tune_pw(h, a);      // per-shape tile choice, timed once (as in inference)
            launch_pw(a, st);
            T.recs.push_back(r);
        }
    }
    if (T.oom) return fail(h, "training workspace exhausted (%zu bytes)", h->train_arena_bytes);
    if (h->fwd_only[0]) {                                  // yn_train_forward: raw heads as dense fp32 rows, nothing else
        for (int k = 0; k < 3; ++k) launch_rows_to_f32(hd[k].out, 0, HCp, h->fwd_only[k], h->head_ch, hd[k].M, st);
        HIPCHK(h, hipGetLastError());
        return 0;
    }

    // =============================== loss (+ gradient w.r.t. the raw heads) ===============================
    if (ensure_loss(h, B)) return 1;
    {
        GridInfo g = h->grid;
        g.head_ld = HCp;
        const float* const heads[3] = {hd[0].out, hd[1].out, hd[2].out};
        float* const gheads[3] = {hd[0].gout, hd[1].gout, hd[2].gout};
        // Only the head gradients need zeros (the loss kernel writes the positives' class gradients only, and the pad column).
        // Every activation gradient below is fully written by its FIRST producer (a plain store) before anything
        // accumulates into it — see the first-writer notes at each call — so the region is never memset.
        const char* pe = getenv("YN_TRAIN_POISON");                                            // test hook: NaN-fill first
        const bool poison = pe && atoi(pe);
        if (poison) HIPCHK(h, hipMemsetAsync(T.base + T.cap - T.gused, 0xff, T.gused, st));
        for (int k = 0; k < 3; ++k) HIPCHK(h, hipMemsetAsync(hd[k].gout, 0, (size_t)hd[k].M * HCp * sizeof(float), st));
        launch_loss(nullptr, nullptr, nullptr, heads, gheads, target_dev, g, B, h->loss_partial, losses_dev, nullptr, nullptr, nullptr, st);
    }

    // =============================== backward ===============================
    // heads: every head accumulates into the gradient of its pyramid level
    for (int k = 0; k < 3; ++k) {
        T.back(hd[k].r[4], View{hd[k].gout, HCp, 0, 1}, dense(hd[k].t[3].g, NECK), false);
        for (int j = 3; j >= 1; --j) T.back(hd[k].r[j], dense(hd[k].t[j].g, NECK), dense(hd[k].t[j - 1].g, NECK), false);
        T.back(hd[k].r[0], dense(hd[k].t[0].g, NECK), dense(feats[k].g, NECK), false);      // first writer of p3a / p4b / p5a
    }
    // PAN / FPN (models/yolo_nano.py:291-296), in reverse
    T.back(r_sm3, dense(p5a.g, NECK), dense(d5.g, NECK), false);
    launch_resample(d5.g, nullptr, p4b.g, B, W5, W5, NECK, 3, st);
    T.back(r_sm2, dense(p4b.g, NECK), dense(d4.g, NECK), false);
    launch_resample(d4.g, nullptr, p3a.g, B, W4, W4, NECK, 3, st);
    T.back(r_sm1, dense(p3a.g, NECK), dense(u3.g, NECK), false);
    launch_resample(u3.g, nullptr, p4a.g, B, W3, W3, NECK, 2, st);
    T.back(r_sm0, dense(p4a.g, NECK), dense(u4.g, NECK), false);
    launch_resample(u4.g, nullptr, p5.g, B, W4, W4, NECK, 2, st);
    T.back(r_lat2, dense(p5.g, NECK), dense(cfeat[2].g, h->stage_ch[2]), false);               // laterals: first writers of the stage outputs' gradients
    T.back(r_lat1, dense(p4.g, NECK), dense(cfeat[1].g, h->stage_ch[1]), false);
    T.back(r_lat0, dense(p3.g, NECK), dense(cfeat[0].g, h->stage_ch[0]), false);
    // backbone blocks in reverse (backbone/shufflenetv2.py:69-78)
    for (int bi = (int)blks.size() - 1; bi >= 0; --bi) {
        Blk& k = blks[bi];
        const int C = k.C, bf = k.bf;
        const long Mo = (long)B * k.Hout * k.Hout;
        if (!k.s2) {
            // out[2j] = x1[j] (pass-through), out[2j+1] = branch2[j]
            // k.in is never a stage output: its gradient is written once, [0,bf) by this copy and [bf,C) by pw1's input gradient
            launch_strided_copy(k.out.g, C, 0, 2, k.in.g, C, 0, 1, Mo, bf, 0, st);
            T.back(k.r_pw2, View{k.out.g, C, 1, 2}, dense(k.t2.g, bf), false);
            T.back(k.r_dw, dense(k.t2.g, bf), dense(k.t1.g, bf), false);
            T.back(k.r_pw1, dense(k.t1.g, bf), View{k.in.g, C, bf, 1}, false);
        } else {
            T.back(k.r_pw2, View{k.out.g, C, 1, 2}, dense(k.t2.g, bf), false);
            T.back(k.r_dw, dense(k.t2.g, bf), dense(k.t1.g, bf), false);
            // k.in is the previous stage's output (its lateral wrote the gradient first) or the max-pool output (nobody did)
            T.back(k.r_pw1, dense(k.t1.g, bf), dense(k.in.g, k.Cin), k.in.g != a1.g);
            launch_strided_copy(k.out.g, C, 0, 2, k.tb1.g, bf, 0, 1, Mo, bf, 0, st);         // gradient of branch1's output
            T.back(k.r_b1pw, dense(k.tb1.g, bf), dense(k.tdw1.g, k.Cin), false);
            T.back(k.r_b1dw, dense(k.tdw1.g, k.Cin), dense(k.in.g, k.Cin), true);
        }
    }
    // max pool + stem
    launch_maxpool_bwd(a1.g, pool_idx, B, H1, H1, 24, a0.g, st);
    T.back(r_stem, dense(a0.g, 24), View{nullptr, 0, 0, 1}, false, false);
    T.flush_params();
    if (T.side) {                                          // every weight gradient is in before the slots are combined
        hipEvent_t e = h->train_events[Trainer::NEV];
        HIPCHK(h, hipEventRecord(e, T.side));
        HIPCHK(h, hipStreamWaitEvent(st, e, 0));
    }
    launch_grad_combine(h->tG, T.gslots, (long)h->tN, (size_t)h->tN, st);
    HIPCHK(h, hipGetLastError());

    if (do_update) {
        if (!h->skip_flag) {
            HIPCHK(h, hipMalloc((void**)&h->skip_flag, 2 * sizeof(int)));
            HIPCHK(h, hipMemsetAsync(h->skip_flag, 0, 2 * sizeof(int), st));
        }
        launch_sgd(h->tP, h->tG, h->tM, (long)h->tN, lr, momentum, weight_decay, grad_scale, 0, h->skip_flag, st);   // momentum starts at zero: no first-step case
        h->train_steps++;
        HIPCHK(h, hipGetLastError());
    }
    h->folded = false;                                    // inference packs are stale now
    return 0;
}

// ---- single kernels of the fp16 step behind fp32 tensors (op-level parity tests): inputs are rounded to fp16 into the padded
//      (gapped != 0: two-plane) layout, ONE forward kernel / ONE backward kernel pair runs, results come back as fp32 ----------
int yn_op_h16_conv(yn_handle* h, int kind, const float* x, int B, int H, int W, int Cin, int gapped, const float* w, const float* bias, int Cout, int stride,
                   const float* dy, float* y, float* dx, float* dw)
{
    YN_ENTER(h);
    if (kind < 0 || kind > 2 || !x || !w || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return fail(h, "yn_op_h16_conv: bad arguments");
    if (kind == 1 && Cin != Cout) return fail(h, "yn_op_h16_conv: depthwise needs Cin == Cout");
    if (kind != 1 && stride != 1) return fail(h, "yn_op_h16_conv: only the depthwise conv has a stride");
    if (gapped && (Cin & 1)) return fail(h, "yn_op_h16_conv: a gapped input has an even channel count");
    if ((dx || dw) && !dy) return fail(h, "yn_op_h16_conv: gradients need dy");
    hipStream_t st = h->stream;
    const int half = gapped ? Cin / 2 : Cin, gap = gapped ? r8(half) - half : 0, Cp = gapped ? 2 * r8(half) : r8(Cin);
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const long Mi = (long)B * H * W, Mo = (long)B * Ho * Wo;
    const int taps = kind == 2 ? 9 : 1;
    const int oC = Cout, Np = kind == 1 ? Cp : r8(Cout), ohalf = kind == 1 ? half : Cout, ogap = kind == 1 ? gap : 0;
    DevBuf xb((size_t)Mi * Cp * sizeof(h16), st), yb((size_t)Mo * Np * sizeof(h16), st), dyb((size_t)Mo * Np * sizeof(h16), st), dxb((size_t)Mi * Cp * sizeof(h16), st);
    const int Npad = r32(Cout), Kpb = r8(Cout), Npadb = r32(Cp);
    DevBuf wf((size_t)taps * Cp * Npad * sizeof(h16), st), wb((size_t)taps * Kpb * Npadb * sizeof(h16), st), bb((size_t)(Npad > Cp ? Npad : Cp) * sizeof(float), st);
    DevBuf dwf((size_t)9 * Cp * sizeof(float), st), dwbk((size_t)9 * Cp * sizeof(float), st);
    DevBuf part((size_t)(4 << 20) * sizeof(float), st), slots((size_t)GRAD_SLOTS * Cout * 9 * sizeof(float), st);
    if (!xb.p || !yb.p || !dyb.p || !dxb.p || !wf.p || !wb.p || !bb.p || !dwf.p || !dwbk.p || !part.p || !slots.p) return fail(h, "yn_op_h16_conv: out of memory");
    launch_hstage(x, Cin, xb.as<h16>(), Cp, half, gap, Mi, st);
    if (kind == 1) {
        launch_hpack_dw(w, bias, Cout, half, gap, Cp, 0, dwf.as<float>(), bb.as<float>(), st);
        launch_hpack_dw(w, nullptr, Cout, half, gap, Cp, 1, dwbk.as<float>(), nullptr, st);
        HDwArgs a{};
        a.in = xb.as<h16>(); a.in_ld = Cp; a.w = dwf.as<float>(); a.bias = bb.as<float>(); a.out = yb.as<h16>(); a.out_ld = Np;
        a.B = B; a.H = H; a.W = W; a.Cp = Cp; a.stride = stride;
        launch_hdw(a, st);
    } else {
        launch_hpack_gemm(w, Cout, Cin, taps, half, gap, Cp, Npad, 0, wf.as<h16>(), st);
        launch_hpack_gemm(w, Cout, Cin, taps, half, gap, Kpb, Npadb, 1, wb.as<h16>(), st);
        if (bias) HIPCHK(h, hipMemcpyAsync(bb.p, bias, (size_t)Cout * sizeof(float), hipMemcpyDeviceToDevice, st));
        HGemmArgs a{};
        a.in = xb.as<h16>(); a.in_ld = Cp; a.H = H; a.W = W; a.taps = taps; a.Wp = wf.as<h16>(); a.bias = bb.as<float>();
        a.out = yb.as<h16>(); a.out_ld = Np; a.M = (int)Mo; a.Kp = Cp; a.Np = Np; a.Npad = Npad;
        launch_hgemm(a, st);
    }
    if (y) launch_hunstage(yb.as<h16>(), Np, ohalf, ogap, y, oC, Mo, st);
    if (dy) {
        launch_hstage(dy, oC, dyb.as<h16>(), Np, ohalf, ogap, Mo, st);
        if (dx) {
            if (kind == 1 && stride == 2) launch_hdw_dgrad_s2(dyb.as<h16>(), Np, dwf.as<float>(), B, H, W, Cp, dxb.as<h16>(), Cp, 0, 0, st);
            else if (kind == 1) {
                HDwArgs a{};
                a.in = dyb.as<h16>(); a.in_ld = Np; a.w = dwbk.as<float>(); a.out = dxb.as<h16>(); a.out_ld = Cp; a.B = B; a.H = H; a.W = W; a.Cp = Cp; a.stride = 1;
                launch_hdw(a, st);
            } else {
                HGemmArgs a{};
                a.in = dyb.as<h16>(); a.in_ld = Np; a.H = H; a.W = W; a.taps = taps; a.Wp = wb.as<h16>(); a.out = dxb.as<h16>(); a.out_ld = Cp;
                a.M = (int)Mo; a.Kp = Kpb; a.Np = Cp; a.Npad = Npadb;
                launch_hgemm(a, st);
            }
            launch_hunstage(dxb.as<h16>(), Cp, half, gap, dx, Cin, Mi, st);
        }
        if (dw) {
            if (kind == 1) {
                HIPCHK(h, hipMemsetAsync(dw, 0, (size_t)Cout * 9 * sizeof(float), st));
                launch_hdw_wgrad(dyb.as<h16>(), Np, xb.as<h16>(), Cp, 0, B, H, W, Cout, Cp, half, gap, stride, dw, part.as<float>(), (size_t)4 << 20, st);
            } else {
                HWgradArgs a{};
                a.dy = dyb.as<h16>(); a.dy_ld = Np; a.x = xb.as<h16>(); a.x_ld = Cp; a.H = H; a.W = W; a.taps = taps; a.M = (int)Mo; a.Np = Np; a.Kp = Cp;
                a.N = Cout; a.Cin = Cin; a.half = half; a.gap = gap; a.dw = dw; a.partial = part.as<float>(); a.partial_cap = (size_t)4 << 20;
                launch_hwgrad(a, st);
            }
        }
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(st));                    // the temporaries are freed on return
    return 0;
}

// The HColStat epilogues of hgemm_kernel on their own: forward conv + the column sums of its (fp16) output; input gradient + the
// BatchNorm-backward sums of the layer below.  sums come back as double [2][channels] (the 32 slots collapsed on the host).
int yn_op_h16_gemm_stats(yn_handle* h, int kind, const float* x, int B, int H, int W, int Cin, int gapped, const float* w, int Cout,
                         float* y, double* sums_fwd, const float* dy, const float* y_below, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, int act, float* dx, double* sums_bwd)
{
    YN_ENTER(h);
    if ((kind != 0 && kind != 2) || !x || !w || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || !y || !sums_fwd) return fail(h, "yn_op_h16_gemm_stats: bad arguments");
    if (gapped && (Cin & 1)) return fail(h, "yn_op_h16_gemm_stats: a gapped input has an even channel count");
    if (dy && (!y_below || !mean || !invstd || !gamma || !beta || !dx || !sums_bwd)) return fail(h, "yn_op_h16_gemm_stats: the backward half needs y_below, mean, invstd, gamma, beta, dx, sums_bwd");
    if (Cin > 256 || Cout > 256) return fail(h, "yn_op_h16_gemm_stats: at most 256 channels");
    hipStream_t st = h->stream;
    const int half = gapped ? Cin / 2 : Cin, gap = gapped ? r8(half) - half : 0, Cp = gapped ? 2 * r8(half) : r8(Cin);
    const long M = (long)B * H * W;
    const int taps = kind == 2 ? 9 : 1, Np = r8(Cout), Npad = r32(Cout), Kpb = r8(Cout), Npadb = r32(Cp);
    DevBuf xb((size_t)M * Cp * sizeof(h16), st), yb((size_t)M * Np * sizeof(h16), st), dyb((size_t)M * Np * sizeof(h16), st), dxb((size_t)M * Cp * sizeof(h16), st), ybb((size_t)M * Cp * sizeof(h16), st);
    DevBuf wf((size_t)taps * Cp * Npad * sizeof(h16), st), wb((size_t)taps * Kpb * Npadb * sizeof(h16), st);
    DevBuf accf((size_t)2 * HACC_SLOTS * Cout * sizeof(double), st), accb((size_t)2 * HACC_SLOTS * Cin * sizeof(double), st);
    if (!xb.p || !yb.p || !dyb.p || !dxb.p || !ybb.p || !wf.p || !wb.p || !accf.p || !accb.p) return fail(h, "yn_op_h16_gemm_stats: out of memory");
    launch_hstage(x, Cin, xb.as<h16>(), Cp, half, gap, M, st);
    launch_hpack_gemm(w, Cout, Cin, taps, half, gap, Cp, Npad, 0, wf.as<h16>(), st);
    launch_hpack_gemm(w, Cout, Cin, taps, half, gap, Kpb, Npadb, 1, wb.as<h16>(), st);
    HGemmArgs a{};
    a.in = xb.as<h16>(); a.in_ld = Cp; a.H = H; a.W = W; a.taps = taps; a.Wp = wf.as<h16>(); a.out = yb.as<h16>(); a.out_ld = Np; a.M = (int)M; a.Kp = Cp; a.Np = Np; a.Npad = Npad;
    a.st.acc = accf.as<double>(); a.st.C = Cout; a.st.half = Cout; a.st.gap = 0;
    launch_hgemm(a, st);
    launch_hunstage(yb.as<h16>(), Np, Cout, 0, y, Cout, M, st);
    std::vector<double> host((size_t)2 * HACC_SLOTS * (Cout > Cin ? Cout : Cin));
    HIPCHK(h, hipMemcpyAsync(host.data(), accf.p, (size_t)2 * HACC_SLOTS * Cout * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    for (int k = 0; k < 2 * Cout; ++k) { double v = 0.0; for (int sl = 0; sl < HACC_SLOTS; ++sl) v += host[(size_t)sl * 2 * Cout + k]; sums_fwd[k] = v; }
    if (dy) {
        launch_hstage(dy, Cout, dyb.as<h16>(), Np, Cout, 0, M, st);
        launch_hstage(y_below, Cin, ybb.as<h16>(), Cp, half, gap, M, st);
        HGemmArgs b{};
        b.in = dyb.as<h16>(); b.in_ld = Np; b.H = H; b.W = W; b.taps = taps; b.Wp = wb.as<h16>(); b.out = dxb.as<h16>(); b.out_ld = Cp; b.M = (int)M; b.Kp = Kpb; b.Np = Cp; b.Npad = Npadb;
        b.st.acc = accb.as<double>(); b.st.C = Cin; b.st.half = half; b.st.gap = gap; b.st.y = ybb.as<h16>(); b.st.y_ld = Cp;
        b.st.mean = mean; b.st.invstd = invstd; b.st.gamma = gamma; b.st.beta = beta; b.st.act = act;
        launch_hgemm(b, st);
        launch_hunstage(dxb.as<h16>(), Cp, half, gap, dx, Cin, M, st);
        HIPCHK(h, hipMemcpyAsync(host.data(), accb.p, (size_t)2 * HACC_SLOTS * Cin * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        for (int k = 0; k < 2 * Cin; ++k) { double v = 0.0; for (int sl = 0; sl < HACC_SLOTS; ++sl) v += host[(size_t)sl * 2 * Cin + k]; sums_bwd[k] = v; }
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(st));
    return 0;
}

int yn_op_h16_bn(yn_handle* h, const float* y, const float* dz, int64_t M, int C, const float* gamma, const float* beta, int act,
                 float* z, float* dy, float* dgamma, float* dbeta)
{
    YN_ENTER(h);
    if (!y || !gamma || !beta || M <= 0 || C <= 0 || !z) return fail(h, "yn_op_h16_bn: bad arguments");
    if (dz && (!dy || !dgamma || !dbeta)) return fail(h, "yn_op_h16_bn: the backward pass needs dy, dgamma and dbeta");
    hipStream_t st = h->stream;
    const int Cp = r8(C);
    DevBuf yb((size_t)M * Cp * sizeof(h16), st), zb((size_t)M * Cp * sizeof(h16), st), dzb((size_t)M * Cp * sizeof(h16), st), dyb((size_t)M * Cp * sizeof(h16), st);
    DevBuf acc((size_t)4 * HACC_SLOTS * C * sizeof(double), st), mi((size_t)2 * C * sizeof(float), st);
    if (!yb.p || !zb.p || !dzb.p || !dyb.p || !acc.p || !mi.p) return fail(h, "yn_op_h16_bn: out of memory");
    launch_hstage(y, C, yb.as<h16>(), Cp, C, 0, (long)M, st);
    HRedArgs q{};
    q.y = yb.as<h16>(); q.y_ld = Cp; q.M = (int)M; q.C = C; q.Cp = Cp; q.half = C; q.gap = 0; q.acc = acc.as<double>();
    launch_hcol_reduce(q, 0, st);
    HBnApplyArgs a{};
    a.y = yb.as<h16>(); a.y_ld = Cp; a.acc = acc.as<double>(); a.eps = 1e-5f; a.M = (int)M; a.C = C; a.Cp = Cp; a.half = C; a.gap = 0; a.act = act;
    a.mean = mi.as<float>(); a.invstd = mi.as<float>() + C; a.gamma = gamma; a.beta = beta; a.momentum = 0.1f; a.out = zb.as<h16>(); a.out_ld = Cp;
    launch_hbn_apply(a, st);
    launch_hunstage(zb.as<h16>(), Cp, C, 0, z, C, (long)M, st);
    if (dz) {
        launch_hstage(dz, C, dzb.as<h16>(), Cp, C, 0, (long)M, st);
        q.dz = dzb.as<h16>(); q.dz_ld = Cp; q.mean = a.mean; q.invstd = a.invstd; q.gamma = gamma; q.beta = beta; q.act = act;
        q.acc = acc.as<double>() + 2 * HACC_SLOTS * (size_t)C;
        launch_hbn_bwd(q, dyb.as<h16>(), dgamma, dbeta, st);
        launch_hunstage(dyb.as<h16>(), Cp, C, 0, dy, C, (long)M, st);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(st));
    return 0;
}

int yn_op_h16_bn_unit(yn_handle* h, const float* y, const float* pass, const float* dunit, int64_t M, int C, const float* gamma, const float* beta, int act,
                      float* unit, float* dy, float* deven, float* dgamma, float* dbeta)
{
    YN_ENTER(h);
    if (!y || !pass || !gamma || !beta || M <= 0 || C <= 0 || C > 128 || !unit) return fail(h, "yn_op_h16_bn_unit: bad arguments");
    if (dunit && (!dy || !deven || !dgamma || !dbeta)) return fail(h, "yn_op_h16_bn_unit: the backward pass needs dy, deven, dgamma and dbeta");
    hipStream_t st = h->stream;
    const int Cp = r8(C), gap = Cp - C, Up = 2 * Cp;
    DevBuf yb((size_t)M * Cp * sizeof(h16), st), pb((size_t)M * Cp * sizeof(h16), st), ub((size_t)M * Up * sizeof(h16), st), dub((size_t)M * Up * sizeof(h16), st);
    DevBuf dyb((size_t)M * Cp * sizeof(h16), st), evb((size_t)M * Cp * sizeof(h16), st);
    DevBuf acc((size_t)4 * HACC_SLOTS * C * sizeof(double), st), mi((size_t)2 * C * sizeof(float), st);
    if (!yb.p || !pb.p || !ub.p || !dub.p || !dyb.p || !evb.p || !acc.p || !mi.p) return fail(h, "yn_op_h16_bn_unit: out of memory");
    launch_hstage(y, C, yb.as<h16>(), Cp, C, 0, (long)M, st);
    launch_hstage(pass, C, pb.as<h16>(), Cp, C, 0, (long)M, st);
    HRedArgs q{};
    q.y = yb.as<h16>(); q.y_ld = Cp; q.M = (int)M; q.C = C; q.Cp = Cp; q.half = C; q.gap = 0; q.acc = acc.as<double>();
    launch_hcol_reduce(q, 0, st);
    HBnApplyArgs a{};
    a.y = yb.as<h16>(); a.y_ld = Cp; a.acc = acc.as<double>(); a.eps = 1e-5f; a.M = (int)M; a.C = C; a.Cp = Cp; a.half = C; a.gap = 0; a.act = act;
    a.mean = mi.as<float>(); a.invstd = mi.as<float>() + C; a.gamma = gamma; a.beta = beta; a.momentum = 0.1f;
    a.out = ub.as<h16>(); a.out_ld = Up; a.pass = pb.as<h16>(); a.pass_ld = Cp; a.out_half = C; a.out_gap = gap;
    launch_hbn_apply(a, st);
    launch_hunstage(ub.as<h16>(), Up, C, gap, unit, 2 * C, (long)M, st);
    if (dunit) {
        launch_hstage(dunit, 2 * C, dub.as<h16>(), Up, C, gap, (long)M, st);
        q.dz = dub.as<h16>(); q.dz_ld = Up; q.dz_odd = 1; q.dz_half = C; q.dz_gap = gap;
        q.mean = a.mean; q.invstd = a.invstd; q.gamma = gamma; q.beta = beta; q.act = act;
        q.acc = acc.as<double>() + 2 * HACC_SLOTS * (size_t)C;
        q.even = evb.as<h16>(); q.even_ld = Cp;
        launch_hbn_bwd(q, dyb.as<h16>(), dgamma, dbeta, st);
        launch_hunstage(dyb.as<h16>(), Cp, C, 0, dy, C, (long)M, st);
        launch_hunstage(evb.as<h16>(), Cp, C, 0, deven, C, (long)M, st);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(st));
    return 0;
}

int yn_train_forward(yn_handle* h, const float* x_dev, int B, float* head_s8, float* head_s16, float* head_s32)
{
    YN_ENTER(h);
    if (!head_s8 || !head_s16 || !head_s32) return fail(h, "yn_train_forward: null output");
    h->fwd_only[0] = head_s8; h->fwd_only[1] = head_s16; h->fwd_only[2] = head_s32;
    const int rc = yn_train_step(h, x_dev, nullptr, B, 0.0f, 0.0f, 0.0f, 1.0f, 0, nullptr);
    h->fwd_only[0] = h->fwd_only[1] = h->fwd_only[2] = nullptr;
    return rc;
}

int yn_train_precision(yn_handle* h, int dtype)
{
    YN_ENTER(h);
    if (dtype != YN_F32 && dtype != YN_F16) return fail(h, "yn_train_precision: unknown dtype %d", dtype);
    h->train_dtype = dtype;
    return 0;
}

int yn_train_graph(yn_handle* h, int enable, int64_t* replays)
{
    YN_ENTER(h);
    if (enable >= 0) {
        if (!enable) drop_train_graphs(h);
        h->train_graph = enable != 0;
    }
    if (replays) *replays = h->train_graph_replays;
    return 0;
}

int yn_train_skipped_steps(yn_handle* h, int64_t* count)
{
    YN_ENTER(h);
    if (!count) return fail(h, "yn_train_skipped_steps: null output");
    int v[2] = {0, 0};
    if (h->skip_flag) {
        HIPCHK(h, hipMemcpyAsync(v, h->skip_flag, sizeof v, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    *count = v[1];
    return 0;
}

// The fp16 step runs the head towers of levels 3 / 4 on fork streams when that measured faster on THIS device (steps 3-6 of a handle time
// the step both ways): the decision, so that a run can be reproduced (force > 0: pin it to `force - 1`).  *decision: -1 undecided yet, 0 one stream, 1 forked.
int yn_train_head_fork(yn_handle* h, int force, int* decision)
{
    YN_ENTER(h);
    if (force < 0 || force > 2) return fail(h, "yn_train_head_fork: force must be 0 (query), 1 (one stream) or 2 (forked)");
    if (force > 0 && h->head_fork != force - 1) { h->head_fork = force - 1; drop_train_graphs(h); }
    if (decision) *decision = h->head_fork;
    return 0;
}

// ---- the gradient exchange over RCCL, without torch (SURVEY 8(b): yn_allreduce_grads(h, ncclComm_t); train.py:13-14 imports DDP) ----
// The library links only libamdhip64.  RCCL is resolved at run time from whatever librccl the PROCESS already carries (a
// communicator belongs to the library instance that created it: torch bundles its own librccl.so, a C consumer links ROCm's), and
// only then from the system's librccl.so.1.
namespace {
typedef int (*nccl_allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef const char* (*nccl_errstr_fn)(int);
nccl_allreduce_fn g_nccl_allreduce = nullptr;
nccl_errstr_fn g_nccl_errstr = nullptr;
bool resolve_rccl()
{
    if (g_nccl_allreduce) return true;
    void* sym = dlsym(RTLD_DEFAULT, "ncclAllReduce");
    void* lib = nullptr;
    if (!sym) {
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (lib) break;
        }
        if (lib) sym = dlsym(lib, "ncclAllReduce");
    }
    if (!sym) return false;
    g_nccl_allreduce = (nccl_allreduce_fn)sym;
    g_nccl_errstr = (nccl_errstr_fn)(lib ? dlsym(lib, "ncclGetErrorString") : dlsym(RTLD_DEFAULT, "ncclGetErrorString"));
    return true;
}
}  // namespace

int yn_allreduce_grads(yn_handle* h, void* nccl_comm)
{
    YN_ENTER(h);
    if (!nccl_comm) return fail(h, "yn_allreduce_grads: null communicator");
    if (!h->tG || h->tN <= 0) return fail(h, "yn_allreduce_grads before yn_train_bind");
    if (!resolve_rccl()) return fail(h, "yn_allreduce_grads: no RCCL in this process and librccl.so.1 cannot be loaded (%s)", dlerror());
    // ncclFloat32 = 7, ncclSum = 0 (rccl.h); in place, on the handle's stream: ordered after the backward pass, before yn_sgd_step
    const int rc = g_nccl_allreduce(h->tG, h->tG, (size_t)h->tN, 7, 0, nccl_comm, h->stream);
    if (rc != 0) return fail(h, "ncclAllReduce failed: %s (%d)", g_nccl_errstr ? g_nccl_errstr(rc) : "?", rc);
    return 0;
}

// copy a state-dict entry (trainable: from the flat buffer; running statistics: from the handle) to the host
int yn_read_param(yn_handle* h, const char* key, float* host, int64_t numel)
{
    YN_ENTER(h);
    const Param* p = find_param(h, key);
    if (!p) return fail(h, "unknown parameter '%s'", key);
    if ((int64_t)p->numel != numel) return fail(h, "yn_read_param(%s): expected %zu elements", key, p->numel);
    const float* src = (const float*)p->dev;
    auto it = h->toff.find(key);
    if (h->tP && it != h->toff.end()) src = h->tP + it->second;
    HIPCHK(h, hipMemcpyAsync(host, src, p->numel * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
