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

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

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
    Scratch xb((size_t)Mi * Cp * sizeof(h16), st), yb((size_t)Mo * Np * sizeof(h16), st), dyb((size_t)Mo * Np * sizeof(h16), st), dxb((size_t)Mi * Cp * sizeof(h16), st);
    const int Npad = r32(Cout), Kpb = r8(Cout), Npadb = r32(Cp);
    Scratch wf((size_t)taps * Cp * Npad * sizeof(h16), st), wb((size_t)taps * Kpb * Npadb * sizeof(h16), st), bb((size_t)(Npad > Cp ? Npad : Cp) * sizeof(float), st);
    Scratch dwf((size_t)9 * Cp * sizeof(float), st), dwbk((size_t)9 * Cp * sizeof(float), st);
    Scratch part((size_t)(4 << 20) * sizeof(float), st), slots((size_t)GRAD_SLOTS * Cout * 9 * sizeof(float), st);
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
    Scratch yb((size_t)M * Cp * sizeof(h16), st), zb((size_t)M * Cp * sizeof(h16), st), dzb((size_t)M * Cp * sizeof(h16), st), dyb((size_t)M * Cp * sizeof(h16), st);
    Scratch acc((size_t)4 * HACC_SLOTS * C * sizeof(double), st), mi((size_t)2 * C * sizeof(float), st);
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
    Scratch yb((size_t)M * Cp * sizeof(h16), st), pb((size_t)M * Cp * sizeof(h16), st), ub((size_t)M * Up * sizeof(h16), st), dub((size_t)M * Up * sizeof(h16), st);
    Scratch dyb((size_t)M * Cp * sizeof(h16), st), evb((size_t)M * Cp * sizeof(h16), st);
    Scratch acc((size_t)4 * HACC_SLOTS * C * sizeof(double), st), mi((size_t)2 * C * sizeof(float), st);
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

}  // extern "C"
#pragma GCC visibility pop
