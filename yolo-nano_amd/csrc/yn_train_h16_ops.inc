// yn_train_h16_ops.inc — single kernels of the fp16 training step behind fp32 tensors (op-level parity tests), included by yn_api.hip
// after yn_train_h16.inc, whose channel-map helpers they use.

namespace {

// scratch of the op-level entry points (yn_op_h16_*, yn_op_f32_*), filled with the byte `fill` (zero; 0xff makes every float a NaN), freed on scope exit
struct Scratch {
    DevBuf<char> buf;
    void* p = nullptr;                                      // null: the allocation failed
    explicit Scratch(size_t bytes, hipStream_t st, int fill = 0)
    {
        if (buf.reserve(bytes ? bytes : 16)) return;
        p = buf;
        (void)hipMemsetAsync(p, fill, buf.cap(), st);
    }
    template <class T> T* as() { return (T*)p; }
};

// logical channels -> the step's physical row: dense (gap 0) or the two planes of a ShuffleV2 unit tensor
struct HOpMap { int C, half, gap, Cp; };
inline HOpMap hop_map(int C, bool two_planes)
{
    HOpMap m;
    m.C = C; m.half = two_planes ? C / 2 : C; m.gap = two_planes ? r8(m.half) - m.half : 0; m.Cp = two_planes ? 2 * r8(m.half) : r8(C);
    return m;
}
// a conv operand as the op entries take it: C channels of an fp32 row of ld floats starting at off - the whole row (ld == C, off == 0; two-plane if
// `gapped`), or one plane of a two-plane tensor (ld == 2 C, off == 0 | C: what pw1 / the depthwise conv of a stride-1 unit read and write)
struct HOpView { HOpMap row, view; int pld, poff; };      // row: map of the staged tensor; view: map of the conv's channels; physical row stride and offset
inline bool hop_view(int C, int gapped, int ld, int off, HOpView& v)
{
    if (ld == C && off == 0) { v.row = v.view = hop_map(C, gapped != 0); v.pld = v.row.Cp; v.poff = 0; return true; }
    if (!gapped && ld == 2 * C && (off == 0 || off == C)) {
        v.row = hop_map(2 * C, true); v.view = hop_map(C, false); v.pld = v.row.Cp; v.poff = off ? v.view.Cp : 0;
        return true;
    }
    return false;
}

// g[n] = the step's combine of a flat gradient: (g + sum of the GRAD_SLOTS slot copies) / S with S = 1 (hgrad_finish_kernel on a state of its own)
int hop_finish(yn_handle* h, float* g, const float* slots, long n, hipStream_t st)
{
    Scratch state(5 * sizeof(float), st);
    if (!state.p) return fail(h, "out of memory");
    const float one[2] = {1.0f, 1.0f};
    HIPCHK(h, hipMemcpyAsync(state.p, one, sizeof(one), hipMemcpyHostToDevice, st));
    {
        Bracket br(h, "op.h16.finish", 0.0, 0.0);
        launch_hgrad_finish(g, slots, n, (size_t)n, state.as<float>(), st);
    }
    HIPCHK(h, hipStreamSynchronize(st));
    return 0;
}

int hop_sums_to_host(yn_handle* h, const double* acc_dev, int C, double* sums, hipStream_t st)
{
    std::vector<double> host((size_t)2 * HACC_SLOTS * C);
    HIPCHK(h, hipMemcpyAsync(host.data(), acc_dev, host.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    for (int k = 0; k < 2 * C; ++k) { double v = 0.0; for (int sl = 0; sl < HACC_SLOTS; ++sl) v += host[(size_t)sl * 2 * C + k]; sums[k] = v; }
    return 0;
}

constexpr size_t HOP_PART_FLOATS = (size_t)4 << 20;         // the weight-gradient scratch of the op entries

int op_h16_conv(yn_handle* h, const char* who, int kind, const float* x, int B, int H, int W, int Cin, int gapped, int x_ld, int x_off,
                const float* w, const float* bias, int Cout, int stride, const float* dy, int accumulate, int dx_ld, int dx_off, int64_t partial_cap,
                int stat, const float* y_below, const float* mean, const float* invstd, const float* gamma, const float* beta, int act,
                float* y, float* dx, float* dw, float* dbias, double* sums_fwd, double* sums_bwd)
{
    if (kind < 0 || kind > 2 || !x || !w || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return fail(h, "%s: bad arguments", who);
    if (kind == 1 && Cin != Cout) return fail(h, "%s: depthwise needs Cin == Cout", who);
    if (kind == 1 ? (stride != 1 && stride != 2) : stride != 1) return fail(h, "%s: only the depthwise conv has a stride (1 or 2)", who);
    if (gapped && (Cin & 1)) return fail(h, "%s: a gapped input has an even channel count", who);
    if ((dx || dw || dbias) && !dy) return fail(h, "%s: gradients need dy", who);
    if ((long)B * H * W > 0x7fffffffL / 512) return fail(h, "%s: at most 2^22 pixels", who);
    HOpView xv, dv;
    if (!hop_view(Cin, gapped, x_ld, x_off, xv)) return fail(h, "%s: x is the whole row (x_ld = Cin, x_off = 0) or one plane of an ungapped two-plane tensor (x_ld = 2 Cin, x_off = 0 | Cin): every other slice starts off a 16-byte boundary", who);
    if (dx && !hop_view(Cin, gapped, dx_ld, dx_off, dv)) return fail(h, "%s: dx is the whole row (dx_ld = Cin, dx_off = 0) or one plane of an ungapped two-plane tensor (dx_ld = 2 Cin, dx_off = 0 | Cin)", who);
    const HOpMap in = xv.view;
    const HOpMap out = kind == 1 ? in : hop_map(Cout, false);      // the depthwise output keeps its input's channel map
    const int Cp = in.Cp, Np = out.Cp;
    const int taps = kind == 2 ? 9 : 1;
    const size_t wn = kind == 1 ? (size_t)Cout * 9 : (size_t)Cout * Cin * taps;
    const size_t one_copy = kind == 1 ? (size_t)Cout * 9 : (size_t)Np * Cp * taps;
    const size_t cap = partial_cap > 0 ? (size_t)partial_cap : HOP_PART_FLOATS;
    if (partial_cap < 0 || cap > HOP_PART_FLOATS || (dw && cap < one_copy)) return fail(h, "%s: partial_cap holds at least one copy of the packed dw and at most the entry's scratch of 4 Mi floats", who);
    if ((dw && kind == 1 && Np > 256) || (dbias && Np > 256))
        return fail(h, "%s: dw of a depthwise conv and dbias need at most 256 padded channels (hdw_wgrad_kernel and hcol_reduce_kernel combine at most 32 octet lanes)", who);
    if (stat < 0 || stat > 2 || act < 0 || act > 2) return fail(h, "%s: stat is 0, 1 or 2 and act 0, 1 or 2", who);
    if (stat && (kind != 1 || stride != 1 || Cp > 256)) return fail(h, "%s: the statistics forms belong to the stride-1 depthwise run kernel (at most 256 padded channels); yn_op_h16_gemm_stats has the GEMM's", who);
    if (stat == 1 && !sums_fwd) return fail(h, "%s: stat 1 needs sums_fwd", who);
    if (stat == 2 && (!dx || !y_below || !mean || !invstd || !gamma || !beta || !sums_bwd)) return fail(h, "%s: stat 2 needs dy, dx, y_below, mean, invstd, gamma, beta and sums_bwd", who);
    if (stat == 2 && (accumulate || dx_ld != Cin)) return fail(h, "%s: the backward sums are taken of a complete, dense dx (no accumulate, dx_ld = Cin)", who);
    hipStream_t st = h->stream;
    h->cur = st;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const long Mi = (long)B * H * W, Mo = (long)B * Ho * Wo;
    const size_t n = wn + (size_t)Cout;                     // the flat gradient of this one layer: [weight][bias]
    Scratch xb((size_t)Mi * xv.pld * sizeof(h16), st), yb((size_t)Mo * Np * sizeof(h16), st), dyb((size_t)Mo * Np * sizeof(h16), st);
    Scratch dxb(dx ? (size_t)Mi * dv.pld * sizeof(h16) : 0, st), ybb(stat == 2 ? (size_t)Mi * Cp * sizeof(h16) : 0, st);
    const int Npad = r32(Cout), Kpb = r8(Cout), Npadb = r32(Cp);
    Scratch wf((size_t)taps * Cp * Npad * sizeof(h16), st), wb((size_t)taps * Kpb * Npadb * sizeof(h16), st), bb((size_t)(Npad > Cp ? Npad : Cp) * sizeof(float), st);
    Scratch dwf((size_t)9 * Cp * sizeof(float), st), dwbk((size_t)9 * Cp * sizeof(float), st);
    Scratch part((size_t)cap * sizeof(float), st, 0xff), g(n * sizeof(float), st), slots((size_t)GRAD_SLOTS * n * sizeof(float), st);      // the step's partial scratch is not zeroed either
    Scratch acc((size_t)4 * HACC_SLOTS * Cin * sizeof(double), st);
    if (!xb.p || !yb.p || !dyb.p || !dxb.p || !ybb.p || !wf.p || !wb.p || !bb.p || !dwf.p || !dwbk.p || !part.p || !g.p || !slots.p || !acc.p) return fail(h, "%s: out of memory", who);
    launch_hstage(x, xv.row.C, xb.as<h16>(), xv.pld, xv.row.half, xv.row.gap, Mi, st);
    if (kind == 1) {
        launch_hpack_dw(w, bias, Cout, in.half, in.gap, Cp, 0, dwf.as<float>(), bb.as<float>(), st);
        launch_hpack_dw(w, nullptr, Cout, in.half, in.gap, Cp, 1, dwbk.as<float>(), nullptr, st);
        HDwArgs a{};
        a.in = xb.as<h16>(); a.in_ld = xv.pld; a.in_off = xv.poff; a.w = dwf.as<float>(); a.bias = bb.as<float>(); a.out = yb.as<h16>(); a.out_ld = Np;
        a.B = B; a.H = H; a.W = W; a.Cp = Cp; a.stride = stride;
        if (stat == 1) { a.st.acc = acc.as<double>(); a.st.C = out.C; a.st.half = out.half; a.st.gap = out.gap; }
        Bracket br(h, "op.h16.fwd", 2.0 * Mo * 9 * Cout, 0.0);
        launch_hdw(a, st);
    } else {
        launch_hpack_gemm(w, Cout, Cin, taps, in.half, in.gap, Cp, Npad, 0, wf.as<h16>(), st);
        launch_hpack_gemm(w, Cout, Cin, taps, in.half, in.gap, Kpb, Npadb, 1, wb.as<h16>(), st);
        if (bias) HIPCHK(h, hipMemcpyAsync(bb.p, bias, (size_t)Cout * sizeof(float), hipMemcpyDeviceToDevice, st));
        HGemmArgs a{};
        a.in = xb.as<h16>(); a.in_ld = xv.pld; a.in_off = xv.poff; a.H = H; a.W = W; a.taps = taps; a.Wp = wf.as<h16>(); a.bias = bb.as<float>();
        a.out = yb.as<h16>(); a.out_ld = Np; a.M = (int)Mo; a.Kp = Cp; a.Np = Np; a.Npad = Npad;
        Bracket br(h, "op.h16.fwd", 2.0 * Mo * taps * Cin * Cout, 0.0);
        launch_hgemm(a, st);
    }
    if (y) launch_hunstage(yb.as<h16>(), Np, out.half, out.gap, y, out.C, Mo, st);
    if (stat == 1 && hop_sums_to_host(h, acc.as<double>(), out.C, sums_fwd, st)) return 1;
    if (dy) {
        launch_hstage(dy, out.C, dyb.as<h16>(), Np, out.half, out.gap, Mo, st);
        if (dx) {
            launch_hstage(dx, dv.row.C, dxb.as<h16>(), dv.pld, dv.row.half, dv.row.gap, Mi, st);      // the prior contents: added to (accumulate), or kept outside the conv's plane
            if (kind == 1 && stride == 2) {
                Bracket br(h, "op.h16.dx", 0.0, 0.0);
                launch_hdw_dgrad_s2(dyb.as<h16>(), Np, dwf.as<float>(), B, H, W, Cp, dxb.as<h16>(), dv.pld, dv.poff, accumulate ? 1 : 0, st);
            } else if (kind == 1) {
                HDwArgs a{};
                a.in = dyb.as<h16>(); a.in_ld = Np; a.w = dwbk.as<float>(); a.out = dxb.as<h16>(); a.out_ld = dv.pld; a.out_off = dv.poff;
                a.B = B; a.H = H; a.W = W; a.Cp = Cp; a.stride = 1; a.accumulate = accumulate ? 1 : 0;
                if (stat == 2) {
                    launch_hstage(y_below, in.C, ybb.as<h16>(), Cp, in.half, in.gap, Mi, st);
                    a.st.acc = acc.as<double>() + 2 * HACC_SLOTS * (size_t)Cin; a.st.C = in.C; a.st.half = in.half; a.st.gap = in.gap; a.st.y = ybb.as<h16>(); a.st.y_ld = Cp;
                    a.st.mean = mean; a.st.invstd = invstd; a.st.gamma = gamma; a.st.beta = beta; a.st.act = act;
                }
                Bracket br(h, "op.h16.dx", 0.0, 0.0);
                launch_hdw(a, st);
            } else {
                HGemmArgs a{};
                a.in = dyb.as<h16>(); a.in_ld = Np; a.H = H; a.W = W; a.taps = taps; a.Wp = wb.as<h16>(); a.out = dxb.as<h16>(); a.out_ld = dv.pld; a.out_off = dv.poff;
                a.M = (int)Mo; a.Kp = Kpb; a.Np = Cp; a.Npad = Npadb; a.accumulate = accumulate ? 1 : 0;
                Bracket br(h, "op.h16.dx", 0.0, 0.0);
                launch_hgemm(a, st);
            }
            launch_hunstage(dxb.as<h16>(), dv.pld, dv.row.half, dv.row.gap, dx, dv.row.C, Mi, st);
            if (stat == 2 && hop_sums_to_host(h, acc.as<double>() + 2 * HACC_SLOTS * (size_t)Cin, in.C, sums_bwd, st)) return 1;
        }
        if (dbias) {                                          // the bias gradient as the step forms it: column sums of dy into the gradient slots
            HRedArgs q{};
            q.y = dyb.as<h16>(); q.y_ld = Np; q.M = (int)Mo; q.C = out.C; q.Cp = Np; q.half = out.half; q.gap = out.gap;
            q.facc = slots.as<float>() + wn; q.slot_stride = n;
            Bracket br(h, "op.h16.dbias", 0.0, 0.0);
            launch_hcol_reduce(q, 3, st);
        }
        if (dw) {
            if (kind == 1) {
                Bracket br(h, "op.h16.dw", 0.0, 0.0);
                launch_hdw_wgrad(dyb.as<h16>(), Np, xb.as<h16>(), xv.pld, xv.poff, B, H, W, Cout, Cp, in.half, in.gap, stride, slots.as<float>(), part.as<float>(), cap, st);
            } else {
                HWgradArgs a{};
                a.dy = dyb.as<h16>(); a.dy_ld = Np; a.x = xb.as<h16>(); a.x_ld = xv.pld; a.x_off = xv.poff; a.H = H; a.W = W; a.taps = taps; a.M = (int)Mo; a.Np = Np; a.Kp = Cp;
                a.N = Cout; a.Cin = Cin; a.half = in.half; a.gap = in.gap; a.dw = g.as<float>(); a.partial = part.as<float>(); a.partial_cap = cap;
                Bracket br(h, "op.h16.dw", 0.0, 0.0);
                launch_hwgrad(a, st);
            }
        }
        if (dw || dbias) {
            if (hop_finish(h, g.as<float>(), slots.as<float>(), (long)n, st)) return 1;
            if (dw) HIPCHK(h, hipMemcpyAsync(dw, g.p, wn * sizeof(float), hipMemcpyDeviceToDevice, st));
            if (dbias) HIPCHK(h, hipMemcpyAsync(dbias, g.as<float>() + wn, (size_t)Cout * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(st));                    // the temporaries are freed on return
    return 0;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

// ---- single kernels of the fp16 step behind fp32 tensors (op-level parity tests): inputs are rounded to fp16 into the padded
//      (gapped != 0: two-plane) layout, ONE forward kernel / ONE backward kernel per result runs, results come back as fp32.  Every
//      launch under test sits in a Bracket of its own: with yn_profile_enable the records list the kernels that ran, in order. -----------
int yn_op_h16_conv2(yn_handle* h, int kind, const float* x, int B, int H, int W, int Cin, int gapped, int x_ld, int x_off,
                    const float* w, const float* bias, int Cout, int stride, const float* dy, int accumulate, int dx_ld, int dx_off, int64_t partial_cap,
                    int stat, const float* y_below, const float* mean, const float* invstd, const float* gamma, const float* beta, int act,
                    float* y, float* dx, float* dw, float* dbias, double* sums_fwd, double* sums_bwd)
{
    YN_ENTER(h);
    return op_h16_conv(h, "yn_op_h16_conv2", kind, x, B, H, W, Cin, gapped, x_ld, x_off, w, bias, Cout, stride, dy, accumulate, dx_ld, dx_off, partial_cap,
                       stat, y_below, mean, invstd, gamma, beta, act, y, dx, dw, dbias, sums_fwd, sums_bwd);
}

// the first form: dense x and dx, nothing accumulated, the whole scratch, no statistics, no bias gradient
int yn_op_h16_conv(yn_handle* h, int kind, const float* x, int B, int H, int W, int Cin, int gapped, const float* w, const float* bias, int Cout, int stride,
                   const float* dy, float* y, float* dx, float* dw)
{
    YN_ENTER(h);
    if (dx && B > 0 && H > 0 && W > 0 && Cin > 0) HIPCHK(h, hipMemsetAsync(dx, 0, (size_t)B * H * W * Cin * sizeof(float), h->stream));      // (conv2 reads dx's prior contents)
    return op_h16_conv(h, "yn_op_h16_conv", kind, x, B, H, W, Cin, gapped, Cin, 0, w, bias, Cout, stride, dy, 0, Cin, 0, 0,
                       0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, y, dx, dw, nullptr, nullptr, nullptr);
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
    h->cur = st;
    const int half = gapped ? Cin / 2 : Cin, gap = gapped ? r8(half) - half : 0, Cp = gapped ? 2 * r8(half) : r8(Cin);
    const long M = (long)B * H * W;
    const int taps = kind == 2 ? 9 : 1, Np = r8(Cout), Npad = r32(Cout), Kpb = r8(Cout), Npadb = r32(Cp);
    Scratch xb((size_t)M * Cp * sizeof(h16), st), yb((size_t)M * Np * sizeof(h16), st), dyb((size_t)M * Np * sizeof(h16), st), dxb((size_t)M * Cp * sizeof(h16), st), ybb((size_t)M * Cp * sizeof(h16), st);
    Scratch wf((size_t)taps * Cp * Npad * sizeof(h16), st), wb((size_t)taps * Kpb * Npadb * sizeof(h16), st);
    Scratch accf((size_t)2 * HACC_SLOTS * Cout * sizeof(double), st), accb((size_t)2 * HACC_SLOTS * Cin * sizeof(double), st);
    if (!xb.p || !yb.p || !dyb.p || !dxb.p || !ybb.p || !wf.p || !wb.p || !accf.p || !accb.p) return fail(h, "yn_op_h16_gemm_stats: out of memory");
    launch_hstage(x, Cin, xb.as<h16>(), Cp, half, gap, M, st);
    launch_hpack_gemm(w, Cout, Cin, taps, half, gap, Cp, Npad, 0, wf.as<h16>(), st);
    launch_hpack_gemm(w, Cout, Cin, taps, half, gap, Kpb, Npadb, 1, wb.as<h16>(), st);
    HGemmArgs a{};
    a.in = xb.as<h16>(); a.in_ld = Cp; a.H = H; a.W = W; a.taps = taps; a.Wp = wf.as<h16>(); a.out = yb.as<h16>(); a.out_ld = Np; a.M = (int)M; a.Kp = Cp; a.Np = Np; a.Npad = Npad;
    a.st.acc = accf.as<double>(); a.st.C = Cout; a.st.half = Cout; a.st.gap = 0;
    {
        Bracket br(h, "op.h16.fwd", 2.0 * M * taps * Cin * Cout, 0.0);
        launch_hgemm(a, st);
    }
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
        {
            Bracket br(h, "op.h16.dx", 2.0 * M * taps * Cin * Cout, 0.0);
            launch_hgemm(b, st);
        }
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
    return yn_op_h16_bn2(h, y, dz, M, C, gamma, beta, act, z, dy, dgamma, dbeta, nullptr, nullptr);
}

int yn_op_h16_bn2(yn_handle* h, const float* y, const float* dz, int64_t M, int C, const float* gamma, const float* beta, int act,
                  float* z, float* dy, float* dgamma, float* dbeta, float* mean, float* invstd)
{
    YN_ENTER(h);
    if (!y || !gamma || !beta || M <= 0 || C <= 0 || !z) return fail(h, "yn_op_h16_bn: bad arguments");
    if (dz && (!dy || !dgamma || !dbeta)) return fail(h, "yn_op_h16_bn: the backward pass needs dy, dgamma and dbeta");
    if (C > 256 || M > 0x7fffffff || act < 0 || act > 2) return fail(h, "yn_op_h16_bn: at most 256 channels (the BatchNorm kernels keep a channel's constants in 256 LDS slots), M below 2^31, act 0, 1 or 2");
    hipStream_t st = h->stream;
    h->cur = st;
    const int Cp = r8(C);
    Scratch yb((size_t)M * Cp * sizeof(h16), st), zb((size_t)M * Cp * sizeof(h16), st), dzb((size_t)M * Cp * sizeof(h16), st), dyb((size_t)M * Cp * sizeof(h16), st);
    Scratch acc((size_t)4 * HACC_SLOTS * C * sizeof(double), st), mi((size_t)2 * C * sizeof(float), st);
    if (!yb.p || !zb.p || !dzb.p || !dyb.p || !acc.p || !mi.p) return fail(h, "yn_op_h16_bn: out of memory");
    launch_hstage(y, C, yb.as<h16>(), Cp, C, 0, (long)M, st);
    HRedArgs q{};
    q.y = yb.as<h16>(); q.y_ld = Cp; q.M = (int)M; q.C = C; q.Cp = Cp; q.half = C; q.gap = 0; q.acc = acc.as<double>();
    {
        Bracket br(h, "op.h16.stats", 0.0, 0.0);
        launch_hcol_reduce(q, 0, st);
    }
    HBnApplyArgs a{};
    a.y = yb.as<h16>(); a.y_ld = Cp; a.acc = acc.as<double>(); a.eps = 1e-5f; a.M = (int)M; a.C = C; a.Cp = Cp; a.half = C; a.gap = 0; a.act = act;
    a.mean = mi.as<float>(); a.invstd = mi.as<float>() + C; a.gamma = gamma; a.beta = beta; a.momentum = 0.1f; a.out = zb.as<h16>(); a.out_ld = Cp;
    {
        Bracket br(h, "op.h16.apply", 0.0, 0.0);
        launch_hbn_apply(a, st);
    }
    launch_hunstage(zb.as<h16>(), Cp, C, 0, z, C, (long)M, st);
    if (mean) HIPCHK(h, hipMemcpyAsync(mean, a.mean, (size_t)C * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (invstd) HIPCHK(h, hipMemcpyAsync(invstd, a.invstd, (size_t)C * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (dz) {
        launch_hstage(dz, C, dzb.as<h16>(), Cp, C, 0, (long)M, st);
        q.dz = dzb.as<h16>(); q.dz_ld = Cp; q.mean = a.mean; q.invstd = a.invstd; q.gamma = gamma; q.beta = beta; q.act = act;
        q.acc = acc.as<double>() + 2 * HACC_SLOTS * (size_t)C;
        {
            Bracket br(h, "op.h16.bwd", 0.0, 0.0);
            launch_hbn_bwd(q, dyb.as<h16>(), dgamma, dbeta, st);
        }
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
    h->cur = st;
    const int Cp = r8(C), gap = Cp - C, Up = 2 * Cp;
    Scratch yb((size_t)M * Cp * sizeof(h16), st), pb((size_t)M * Cp * sizeof(h16), st), ub((size_t)M * Up * sizeof(h16), st), dub((size_t)M * Up * sizeof(h16), st);
    Scratch dyb((size_t)M * Cp * sizeof(h16), st), evb((size_t)M * Cp * sizeof(h16), st);
    Scratch acc((size_t)4 * HACC_SLOTS * C * sizeof(double), st), mi((size_t)2 * C * sizeof(float), st);
    if (!yb.p || !pb.p || !ub.p || !dub.p || !dyb.p || !evb.p || !acc.p || !mi.p) return fail(h, "yn_op_h16_bn_unit: out of memory");
    launch_hstage(y, C, yb.as<h16>(), Cp, C, 0, (long)M, st);
    launch_hstage(pass, C, pb.as<h16>(), Cp, C, 0, (long)M, st);
    HRedArgs q{};
    q.y = yb.as<h16>(); q.y_ld = Cp; q.M = (int)M; q.C = C; q.Cp = Cp; q.half = C; q.gap = 0; q.acc = acc.as<double>();
    {
        Bracket br(h, "op.h16.stats", 0.0, 0.0);
        launch_hcol_reduce(q, 0, st);
    }
    HBnApplyArgs a{};
    a.y = yb.as<h16>(); a.y_ld = Cp; a.acc = acc.as<double>(); a.eps = 1e-5f; a.M = (int)M; a.C = C; a.Cp = Cp; a.half = C; a.gap = 0; a.act = act;
    a.mean = mi.as<float>(); a.invstd = mi.as<float>() + C; a.gamma = gamma; a.beta = beta; a.momentum = 0.1f;
    a.out = ub.as<h16>(); a.out_ld = Up; a.pass = pb.as<h16>(); a.pass_ld = Cp; a.out_half = C; a.out_gap = gap;
    {
        Bracket br(h, "op.h16.apply", 0.0, 0.0);
        launch_hbn_apply(a, st);
    }
    launch_hunstage(ub.as<h16>(), Up, C, gap, unit, 2 * C, (long)M, st);
    if (dunit) {
        launch_hstage(dunit, 2 * C, dub.as<h16>(), Up, C, gap, (long)M, st);
        q.dz = dub.as<h16>(); q.dz_ld = Up; q.dz_odd = 1; q.dz_half = C; q.dz_gap = gap;
        q.mean = a.mean; q.invstd = a.invstd; q.gamma = gamma; q.beta = beta; q.act = act;
        q.acc = acc.as<double>() + 2 * HACC_SLOTS * (size_t)C;
        q.even = evb.as<h16>(); q.even_ld = Cp;
        {
            Bracket br(h, "op.h16.bwd", 0.0, 0.0);
            launch_hbn_bwd(q, dyb.as<h16>(), dgamma, dbeta, st);
        }
        launch_hunstage(dyb.as<h16>(), Cp, C, 0, dy, C, (long)M, st);
        launch_hunstage(evb.as<h16>(), Cp, C, 0, deven, C, (long)M, st);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(st));
    return 0;
}

// ---- the stem conv (3 -> 24, stride 2, fp32 NCHW in) and its weight gradient ----
int yn_op_h16_stem(yn_handle* h, const float* x_nchw, int B, int H, int W, const float* w, const float* bias, const float* dy, float* y, float* dw)
{
    YN_ENTER(h);
    if (!x_nchw || !w || B <= 0 || H <= 0 || W <= 0 || (!y && !dw)) return fail(h, "yn_op_h16_stem: bad arguments");
    if (dw && !dy) return fail(h, "yn_op_h16_stem: dw needs dy");
    if ((long)B * H * W > (long)1 << 28) return fail(h, "yn_op_h16_stem: at most 2^28 input pixels");
    hipStream_t st = h->stream;
    h->cur = st;
    const long Mo = (long)B * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1);
    const size_t n = 24 * 27;
    Scratch wpk(n * sizeof(float), st), yb((size_t)Mo * 24 * sizeof(h16), st), dyb((size_t)Mo * 24 * sizeof(h16), st), g(n * sizeof(float), st), slots((size_t)GRAD_SLOTS * n * sizeof(float), st);
    if (!wpk.p || !yb.p || !dyb.p || !g.p || !slots.p) return fail(h, "yn_op_h16_stem: out of memory");
    launch_hpack_stem(w, wpk.as<float>(), st);
    if (y) {
        {
            Bracket br(h, "op.h16.fwd", 2.0 * Mo * 27 * 24, 0.0);
            launch_hstem(x_nchw, B, H, W, wpk.as<float>(), bias, yb.as<h16>(), st);
        }
        launch_hunstage(yb.as<h16>(), 24, 24, 0, y, 24, Mo, st);
    }
    if (dw) {
        launch_hstage(dy, 24, dyb.as<h16>(), 24, 24, 0, Mo, st);
        {
            Bracket br(h, "op.h16.dw", 2.0 * Mo * 27 * 24, 0.0);
            launch_hstem_wgrad(dyb.as<h16>(), x_nchw, B, H, W, slots.as<float>(), n, st);
        }
        if (hop_finish(h, g.as<float>(), slots.as<float>(), (long)n, st)) return 1;
        HIPCHK(h, hipMemcpyAsync(dw, g.p, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(st));
    return 0;
}

// ---- 3x3 stride-2 max pool with the recorded window position, and its backward ----
int yn_op_h16_maxpool(yn_handle* h, const float* x, int B, int H, int W, int C, const float* dy, float* y, uint8_t* idx, float* dx)
{
    YN_ENTER(h);
    if (!x || B <= 0 || H <= 0 || W <= 0 || C <= 0 || !y || !idx) return fail(h, "yn_op_h16_maxpool: bad arguments");
    if (C & 7) return fail(h, "yn_op_h16_maxpool: C must be a multiple of 8 (a thread loads a channel octet and stores its eight window positions as one 8-byte word)");
    if (!dy != !dx) return fail(h, "yn_op_h16_maxpool: dy and dx come together");
    if ((long)B * H * W > 0x7fffffffL / 512) return fail(h, "yn_op_h16_maxpool: at most 2^22 pixels");
    hipStream_t st = h->stream;
    h->cur = st;
    const long Mi = (long)B * H * W, Mo = (long)B * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1);
    Scratch xb((size_t)Mi * C * sizeof(h16), st), yb((size_t)Mo * C * sizeof(h16), st), ib((size_t)Mo * C, st, 0xff), dyb((size_t)Mo * C * sizeof(h16), st), dxb((size_t)Mi * C * sizeof(h16), st, 0xff);
    if (!xb.p || !yb.p || !ib.p || !dyb.p || !dxb.p) return fail(h, "yn_op_h16_maxpool: out of memory");
    launch_hstage(x, C, xb.as<h16>(), C, C, 0, Mi, st);
    {
        Bracket br(h, "op.h16.fwd", 0.0, 0.0);
        launch_hmaxpool_idx(xb.as<h16>(), B, H, W, C, yb.as<h16>(), ib.as<uint8_t>(), st);
    }
    launch_hunstage(yb.as<h16>(), C, C, 0, y, C, Mo, st);
    HIPCHK(h, hipMemcpyAsync(idx, ib.p, (size_t)Mo * C, hipMemcpyDeviceToDevice, st));
    if (dy) {
        launch_hstage(dy, C, dyb.as<h16>(), C, C, 0, Mo, st);
        {
            Bracket br(h, "op.h16.dx", 0.0, 0.0);
            launch_hmaxpool_bwd(dyb.as<h16>(), ib.as<uint8_t>(), B, H, W, C, dxb.as<h16>(), st);
        }
        launch_hunstage(dxb.as<h16>(), C, C, 0, dx, C, Mi, st);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(st));
    return 0;
}

// ---- the stem's BatchNorm + activation + max pool in one kernel, and its two-phase backward (y: the stem conv's output [B,H,W,24]) ----
int yn_op_h16_stem_pool(yn_handle* h, const float* y, int B, int H, int W, const float* gamma, const float* beta, int act, const float* g1,
                        float* out, uint8_t* idx, float* mean, float* invstd, float* dy, float* dgamma, float* dbeta)
{
    YN_ENTER(h);
    if (!y || B <= 0 || H <= 0 || W <= 0 || !gamma || !beta || act < 0 || act > 2 || !out || !idx || !mean || !invstd) return fail(h, "yn_op_h16_stem_pool: bad arguments");
    if (g1 && (!dy || !dgamma || !dbeta)) return fail(h, "yn_op_h16_stem_pool: the backward pass needs dy, dgamma and dbeta");
    if ((long)B * H * W > 0x7fffffffL / 512) return fail(h, "yn_op_h16_stem_pool: at most 2^22 pixels");
    hipStream_t st = h->stream;
    h->cur = st;
    constexpr int C = 24;
    const long M = (long)B * H * W, Mo = (long)B * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1);
    Scratch yb((size_t)M * C * sizeof(h16), st), ob((size_t)Mo * C * sizeof(h16), st), ib((size_t)Mo * C, st, 0xff), gb((size_t)Mo * C * sizeof(h16), st);
    Scratch acc((size_t)4 * HACC_SLOTS * C * sizeof(double), st);
    if (!yb.p || !ob.p || !ib.p || !gb.p || !acc.p) return fail(h, "yn_op_h16_stem_pool: out of memory");
    launch_hstage(y, C, yb.as<h16>(), C, C, 0, M, st);
    HRedArgs q{};
    q.y = yb.as<h16>(); q.y_ld = C; q.M = (int)M; q.C = C; q.Cp = C; q.half = C; q.gap = 0; q.acc = acc.as<double>();
    {
        Bracket br(h, "op.h16.stats", 0.0, 0.0);
        launch_hcol_reduce(q, 0, st);
    }
    HBnApplyArgs a{};
    a.y = yb.as<h16>(); a.y_ld = C; a.acc = acc.as<double>(); a.eps = 1e-5f; a.M = (int)M; a.C = C; a.Cp = C; a.half = C; a.gap = 0; a.act = act;
    a.mean = mean; a.invstd = invstd; a.gamma = gamma; a.beta = beta; a.momentum = 0.1f;
    {
        Bracket br(h, "op.h16.fwd", 0.0, 0.0);
        launch_hstem_apply_pool(a, B, H, W, ob.as<h16>(), ib.as<uint8_t>(), st);
    }
    launch_hunstage(ob.as<h16>(), C, C, 0, out, C, Mo, st);
    HIPCHK(h, hipMemcpyAsync(idx, ib.p, (size_t)Mo * C, hipMemcpyDeviceToDevice, st));
    if (g1) {
        launch_hstage(g1, C, gb.as<h16>(), C, C, 0, Mo, st);
        q.mean = mean; q.invstd = invstd; q.gamma = gamma; q.beta = beta; q.act = act;
        q.acc = acc.as<double>() + 2 * HACC_SLOTS * (size_t)C;
        {
            Bracket br(h, "op.h16.bwd", 0.0, 0.0);
            launch_hstem_bwd(q, gb.as<h16>(), ib.as<uint8_t>(), B, H, W, yb.as<h16>(), dgamma, dbeta, st);      // dy in place over y, as the step
        }
        launch_hunstage(yb.as<h16>(), C, C, 0, dy, C, M, st);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(st));
    return 0;
}

// ---- the FPN / PAN adds and their accumulating backwards (modes as yn_op_f32_resample; H, W are those of `a`) ----
int yn_op_h16_resample(yn_handle* h, int mode, const float* a, const float* b, float* out, int B, int H, int W, int C)
{
    YN_ENTER(h);
    if (mode < 0 || mode > 3 || !a || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0 || (mode <= 1 && !b)) return fail(h, "yn_op_h16_resample: bad arguments");
    if ((mode == 0 || mode == 2) && ((H | W) & 1)) return fail(h, "yn_op_h16_resample: modes 0 and 2 halve H and W, which must be even");
    if ((long)B * H * W > 0x7fffffffL / 2048) return fail(h, "yn_op_h16_resample: at most 2^20 pixels");
    hipStream_t st = h->stream;
    h->cur = st;
    const int Cp = r8(C);
    const long Ma = (long)B * H * W;
    const long Mother = (mode == 0 || mode == 2) ? Ma / 4 : Ma * 4;      // pixels of the other map: b (modes 0 / 1) or out (modes 2 / 3)
    const long Mout = mode <= 1 ? Ma : Mother;
    Scratch ab((size_t)Ma * Cp * sizeof(h16), st), bb(mode <= 1 ? (size_t)Mother * Cp * sizeof(h16) : 0, st), ob((size_t)Mout * Cp * sizeof(h16), st);
    if (!ab.p || !bb.p || !ob.p) return fail(h, "yn_op_h16_resample: out of memory");
    launch_hstage(a, C, ab.as<h16>(), Cp, C, 0, Ma, st);
    if (mode <= 1) launch_hstage(b, C, bb.as<h16>(), Cp, C, 0, Mother, st);
    else launch_hstage(out, C, ob.as<h16>(), Cp, C, 0, Mout, st);         // the prior contents the mode adds to
    {
        Bracket br(h, "op.h16.resample", 0.0, 0.0);
        launch_hresample(ab.as<h16>(), mode <= 1 ? bb.as<h16>() : nullptr, ob.as<h16>(), B, H, W, Cp, mode, st);
    }
    launch_hunstage(ob.as<h16>(), Cp, C, 0, out, C, Mout, st);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(st));
    return 0;
}

// ---- hgather_kernel with every map argument of its launcher; src [M][src_ld] and dst [M][dst_ld] are PHYSICAL rows (pads included), so the
//      caller sees what the kernel did to the pads and to everything outside its map ----
int yn_op_h16_gather(yn_handle* h, const float* src, int src_ld, int src_off, int src_cs, int src_half, int src_gap,
                     float* dst, int dst_ld, int dst_off, int dst_cs, int dst_half, int dst_gap, int64_t M, int n, int npad)
{
    YN_ENTER(h);
    if (!src || !dst || src_ld <= 0 || dst_ld <= 0 || M <= 0 || n <= 0 || npad < n || src_off < 0 || dst_off < 0 || src_cs <= 0 || dst_cs <= 0 || src_gap < 0 || dst_gap < 0 || src_half < 0 || dst_half < 0)
        return fail(h, "yn_op_h16_gather: bad arguments");
    if (M > ((int64_t)1 << 24) || src_ld > 4096 || dst_ld > 4096) return fail(h, "yn_op_h16_gather: at most 2^24 rows of at most 4096 halves");
    const long sl = (long)src_off + (long)(n - 1) * src_cs, dl = (long)dst_off + (long)(npad - 1) * dst_cs;
    if (sl + (sl >= src_half ? src_gap : 0) >= src_ld) return fail(h, "yn_op_h16_gather: the last source channel lies outside a row of src_ld halves");
    if (dl + (dl >= dst_half ? dst_gap : 0) >= dst_ld) return fail(h, "yn_op_h16_gather: the last destination channel (npad of them) lies outside a row of dst_ld halves");
    hipStream_t st = h->stream;
    h->cur = st;
    Scratch sb((size_t)M * src_ld * sizeof(h16), st), db((size_t)M * dst_ld * sizeof(h16), st);
    if (!sb.p || !db.p) return fail(h, "yn_op_h16_gather: out of memory");
    launch_hstage(src, src_ld, sb.as<h16>(), src_ld, src_ld, 0, (long)M, st);
    launch_hstage(dst, dst_ld, db.as<h16>(), dst_ld, dst_ld, 0, (long)M, st);
    {
        Bracket br(h, "op.h16.gather", 0.0, 0.0);
        launch_hgather(sb.as<h16>(), src_ld, src_off, src_cs, src_half, src_gap, db.as<h16>(), dst_ld, dst_off, dst_cs, dst_half, dst_gap, (long)M, n, npad, st);
    }
    launch_hunstage(db.as<h16>(), dst_ld, dst_ld, 0, dst, dst_ld, (long)M, st);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(st));
    return 0;
}

// ---- the end of an fp16 backward pass: g = (g + the slot copies) / S with the overflow scan (hgrad_finish_kernel), then - update 1: from the local
//      flag, 2: from the bucket-wide flag `global_flag` - the loss-scale decision (hscale_update_kernel).  state: five 32-bit words on the host, in and
//      out: S, 1 / S, clean steps, the overflow flag (an integer bit pattern), pending. ----
int yn_op_h16_grad_finish(yn_handle* h, float* g, const float* slots, int64_t n, float* state, int update, int global_flag)
{
    YN_ENTER(h);
    if (!g || !slots || n <= 0 || n > ((int64_t)1 << 28) || !state || update < 0 || update > 2) return fail(h, "yn_op_h16_grad_finish: bad arguments");
    hipStream_t st = h->stream;
    h->cur = st;
    Scratch sd(5 * sizeof(float), st), gf(2 * sizeof(int), st);
    if (!sd.p || !gf.p) return fail(h, "yn_op_h16_grad_finish: out of memory");
    const int flag[2] = {global_flag, 0};
    HIPCHK(h, hipMemcpyAsync(sd.p, state, 5 * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(gf.p, flag, sizeof(flag), hipMemcpyHostToDevice, st));
    {
        Bracket br(h, "op.h16.finish", 0.0, 0.0);
        launch_hgrad_finish(g, slots, (long)n, (size_t)n, sd.as<float>(), st);
    }
    if (update) {
        Bracket br(h, "op.h16.scale", 0.0, 0.0);
        launch_hscale_update(sd.as<float>(), update == 2 ? gf.as<int>() : nullptr, st);
    }
    HIPCHK(h, hipMemcpyAsync(state, sd.p, 5 * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(st));
    return 0;
}

// ---- the fp16 step's loss (loss_kernel<true, h16> + loss_reduce_kernel) on its own: the dense fp32 raw heads [B,S/s,S/s,A(5+C)] are staged as
//      fp16 rows of the step's physical width (HTrainer::head_ld), the gradient rows are zeroed as the tape zeroes gout_all, the loss scale sits in
//      a state block of its own.  losses [4] (device); g_* (all or none): the head gradients as dense fp32; pad_nonzero (host, may be null): the
//      elements of the fp16 gradient rows' pad columns that are not +0 ----
int yn_op_h16_loss(yn_handle* h, const float* head_s8, const float* head_s16, const float* head_s32, const float* target, int B, float scale,
                   float* losses, float* g_s8, float* g_s16, float* g_s32, int* pad_nonzero)
{
    YN_ENTER(h);
    if (need_square_grid(h, "yn_op_h16_loss")) return 1;
    if (!head_s8 || !head_s16 || !head_s32 || !target || B <= 0 || !losses || !(scale > 0.0f)) return fail(h, "yn_op_h16_loss: bad arguments");
    if ((g_s8 != nullptr) != (g_s16 != nullptr) || (g_s8 != nullptr) != (g_s32 != nullptr)) return fail(h, "yn_op_h16_loss: pass all three gradient buffers or none");
    if (ensure_loss(h, B)) return 1;
    hipStream_t st = h->stream;
    h->cur = st;
    GridInfo g = h->grid;
    const int HC = g.A * (5 + g.C), HCp = HTrainer::head_ld(HC), pad = HCp - HC;
    g.head_ld = HCp;
    const float* const src[3] = {head_s8, head_s16, head_s32};
    float* const dst[3] = {g_s8, g_s16, g_s32};
    long M[3], Mall = 0;
    for (int k = 0; k < 3; ++k) { M[k] = (long)B * g.hw[k]; Mall += M[k]; }
    Scratch hv((size_t)Mall * HCp * sizeof(h16), st), hg(g_s8 ? (size_t)Mall * HCp * sizeof(h16) : 0, st);      // (zero-filled: the value rows' pads, the gradient rows)
    Scratch state(5 * sizeof(float), st), padf(g_s8 && pad ? (size_t)Mall * pad * sizeof(float) : 0, st);
    if (!hv.p || !hg.p || !state.p || !padf.p) return fail(h, "yn_op_h16_loss: out of memory");
    const float sv[2] = {scale, 1.0f / scale};
    HIPCHK(h, hipMemcpyAsync(state.p, sv, sizeof(sv), hipMemcpyHostToDevice, st));
    const h16* heads[3]; h16* gheads[3];
    long off = 0;
    for (int k = 0; k < 3; ++k) {
        heads[k] = hv.as<h16>() + (size_t)off * HCp; gheads[k] = g_s8 ? hg.as<h16>() + (size_t)off * HCp : nullptr;
        launch_hstage(src[k], HC, hv.as<h16>() + (size_t)off * HCp, HCp, HC, 0, M[k], st);
        off += M[k];
    }
    {
        Bracket br(h, "op.h16.loss", 0.0, 0.0);
        launch_loss_h16(heads, g_s8 ? gheads : nullptr, target, g, B, h->loss_partial, losses, state.as<float>(), st);
    }
    int bad = 0;
    if (g_s8) {
        for (int k = 0; k < 3; ++k) launch_rows_to_f32(gheads[k], 1, HCp, dst[k], HC, M[k], st);
        if (pad) {                                              // the pad columns of all three levels (one block of rows) as [Mall][pad] floats
            launch_rows_to_f32(hg.as<h16>() + HC, 1, HCp, padf.as<float>(), pad, Mall, st);
            std::vector<uint32_t> host((size_t)Mall * pad);
            HIPCHK(h, hipMemcpyAsync(host.data(), padf.p, host.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIPCHK(h, hipStreamSynchronize(st));
            for (uint32_t v : host) bad += v != 0u;
        }
    }
    if (pad_nonzero) *pad_nonzero = bad;
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
