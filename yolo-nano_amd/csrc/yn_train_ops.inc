// yn_train_ops.inc — single layers of the fp32 training step on their own (op-level tests against float64), included by yn_api.hip after
// yn_train.inc, whose per-layer launch functions (conv_forward, bn_forward, bn_backward, param_grads, input_grad, even_channels_to) they
// call: the weight packs, the tile and kernel choices, the gradient slots and the BatchNorm accumulators are the step's own.

namespace {

// a layer that exists for one call: geometry + training packs
struct TmpTrainLayer {
    Layer l;
    TrainPack pk;
    yn_handle* h;
    int rc;
    TmpTrainLayer(yn_handle* h_, int kind, int cin, int cout, int stride, bool has_bias) : h(h_)
    {
        l.name = "op"; l.kind = kind; l.cin = cin; l.cout = cout; l.stride = stride; l.has_bias = has_bias;
        rc = alloc_packs(h, l, pk);
    }
    ~TmpTrainLayer() { (void)hipStreamSynchronize(h->stream); }     // then the packs go with pk
};

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int yn_op_f32_conv(yn_handle* h, int kind, const float* x, int B, int H, int W, int Cin, int x_ld, int x_off, const float* w, const float* bias,
                   int Cout, int stride, int y_ld, int64_t partial_cap, const float* dy, int accumulate, float* y, float* dx, float* dw, float* dbias)
{
    YN_ENTER(h);
    if (kind < K_PW || kind > K_STEM || !x || !w || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return fail(h, "yn_op_f32_conv: bad arguments");
    if (kind == K_STEM) {
        if (Cin != 3 || Cout != 24 || stride != 2 || x_ld != 0 || x_off != 0) return fail(h, "yn_op_f32_conv: the stem is 3 -> 24 at stride 2 over an NCHW input (x_ld = x_off = 0)");
        if (dx) return fail(h, "yn_op_f32_conv: the stem has no input gradient");
    } else {
        if (kind == K_DW ? (stride != 1 && stride != 2) : stride != 1) return fail(h, "yn_op_f32_conv: only the depthwise conv has a stride (1 or 2)");
        if (kind == K_DW && Cin != Cout) return fail(h, "yn_op_f32_conv: depthwise needs Cin == Cout");
        if (x_off < 0 || x_off + Cin > x_ld) return fail(h, "yn_op_f32_conv: channels [x_off, x_off + Cin) must lie inside a row of x_ld floats");
        // the forward and input-gradient kernels load channel pairs (8-byte accesses): as every tensor of the network
        if ((Cin | x_ld | x_off) & 1) return fail(h, "yn_op_f32_conv: Cin, x_ld and x_off must be even");
        if (kind == K_DENSE3 && (Cout & 1)) return fail(h, "yn_op_f32_conv: a dense 3x3 conv needs an even Cout");
    }
    // rows of y / dy: dense, or (pointwise only) padded to a multiple of 4 floats as the step stores a BN-less head conv
    if (y_ld != Cout && !(kind == K_PW && y_ld == ((Cout + 3) & ~3))) return fail(h, "yn_op_f32_conv: y_ld is Cout (pointwise: or Cout rounded up to a multiple of 4)");
    if ((dx || dw || dbias) && !dy) return fail(h, "yn_op_f32_conv: gradients need dy");
    if ((Cout & 1) && y_ld == Cout && (dx || dbias)) return fail(h, "yn_op_f32_conv: dx / dbias of an odd Cout need the padded y_ld (channel pairs are loaded)");
    const size_t wn = kind == K_DW ? (size_t)Cout * 9 : (kind == K_PW ? (size_t)Cout * Cin : (size_t)Cout * Cin * 9);
    const size_t cap = partial_cap > 0 ? (size_t)partial_cap : WPART_FLOATS;
    if (cap < (kind == K_DW ? 8 * wn : wn) || cap > WPART_FLOATS) return fail(h, "yn_op_f32_conv: partial_cap holds at least one copy of dw (depthwise: eight) and at most the step's scratch");
    hipStream_t st = h->stream;
    h->cur = st;
    if (zeros_ready(h)) return 1;
    TmpTrainLayer t(h, kind, Cin, Cout, stride, bias != nullptr);
    if (t.rc) return 1;
    fill_packs(t.l, t.pk, w, bias, st);
    TRec r;
    r.l = &t.l; r.x = View{const_cast<float*>(x), x_ld, x_off, 1}; r.B = B; r.H = H; r.W = W; r.x_nchw = kind == K_STEM ? x : nullptr;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    r.Mi = (long)B * H * W; r.Mo = (long)B * Ho * Wo; r.y = y; r.y_ld = y_ld;
    if (y) conv_forward(h, r, t.pk, st);
    if (dy) {
        // a flat gradient buffer of this one layer, [weight][bias], with its GRAD_SLOTS slot copies; the scratch starts as NaNs: the step's is not zeroed either
        const size_t n = wn + (size_t)Cout;
        Scratch g(n * sizeof(float), st), slots((size_t)GRAD_SLOTS * n * sizeof(float), st);
        Scratch part((dw || dbias) ? cap * sizeof(float) : 0, st, 0xff), tmp(dx && accumulate ? (size_t)r.Mi * Cin * sizeof(float) : 0, st, 0xff);
        if (!g.p || !slots.p || !part.p || !tmp.p) return fail(h, "yn_op_f32_conv: out of memory");
        if (dw || dbias) {
            GradPtrs gp{};
            gp.dw = kind == K_DW ? slots.as<float>() : g.as<float>();
            gp.dbias_slots = dbias ? slots.as<float>() + wn : nullptr; gp.slot_stride = n;
            gp.wpart = part.as<float>(); gp.wpart_cap = cap;
            param_grads(r, dy, y_ld, gp, st);
            launch_grad_combine(g.as<float>(), slots.as<float>(), (long)n, n, st);
            if (dw) HIPCHK(h, hipMemcpyAsync(dw, g.p, wn * sizeof(float), hipMemcpyDeviceToDevice, st));
            if (dbias) HIPCHK(h, hipMemcpyAsync(dbias, g.as<float>() + wn, (size_t)Cout * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
        if (dx) input_grad(h, r, t.pk, dy, y_ld, View{dx, x_ld, x_off, 1}, accumulate != 0, tmp.as<float>(), st);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipStreamSynchronize(st));                // the temporaries are freed on return
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_op_f32_bn(yn_handle* h, const float* y, int64_t M, int C, const float* gamma, const float* beta, int act, int unit, const float* pass,
                 float* running_mean, float* running_var, float* z, float* mean, float* invstd,
                 const float* dz, int dz_ld, int dz_off, float* dy, float* deven, float* dgamma, float* dbeta)
{
    YN_ENTER(h);
    if (!y || !gamma || !beta || M <= 0 || M > 0x7fffffff || C <= 0 || act < 0 || act > 2 || !z || !mean || !invstd) return fail(h, "yn_op_f32_bn: bad arguments");
    if (C & 1) return fail(h, "yn_op_f32_bn: C must be even (a lane loads the channel pair (c, c + 1) of a dense row)");
    if (!running_mean != !running_var) return fail(h, "yn_op_f32_bn: running_mean and running_var come together");
    if (unit && (!pass || (C & 1))) return fail(h, "yn_op_f32_bn: the unit form needs the pass-through tensor and an even C");
    if (dz && (!dy || !dgamma || !dbeta || (unit && !deven))) return fail(h, "yn_op_f32_bn: the backward pass needs dy, dgamma and dbeta (unit form: and deven)");
    if (dz && !unit && (dz_off < 0 || dz_off + C > dz_ld)) return fail(h, "yn_op_f32_bn: channels [dz_off, dz_off + C) must lie inside a row of dz_ld floats");
    hipStream_t st = h->stream;
    Layer l;
    l.name = "op"; l.kind = K_PW; l.cin = l.cout = C; l.act = act;
    Scratch acc((size_t)4 * ACC_SLOTS * C * sizeof(double), st);
    if (!acc.p) return fail(h, "yn_op_f32_bn: out of memory");
    TRec r;
    r.l = &l; r.Mo = (long)M; r.y = const_cast<float*>(y); r.y_ld = C; r.mean = mean; r.invstd = invstd; r.acc = acc.as<double>();
    const BnPtrs p{gamma, beta, running_mean, running_var, dgamma, dbeta};
    if (unit) bn_forward(r, p, View{z, 2 * C, 1, 2}, View{const_cast<float*>(pass), C, 0, 1}, st);      // unit[2c] = pass[c], unit[2c+1] = z[c]
    else bn_forward(r, p, View{z, C, 0, 1}, View{nullptr, 0, 0, 1}, st);
    if (dz) {
        // the step's backward overwrites the saved conv output with dy: here it works on a copy
        HIPCHK(h, hipMemcpyAsync(dy, y, (size_t)M * C * sizeof(float), hipMemcpyDeviceToDevice, st));
        r.y = dy;
        if (unit) {
            even_channels_to(dz, 2 * C, (long)M, View{deven, C, 0, 1}, st);
            bn_backward(r, p, View{const_cast<float*>(dz), 2 * C, 1, 2}, st);
        } else bn_backward(r, p, View{const_cast<float*>(dz), dz_ld, dz_off, 1}, st);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(st));
    return 0;
}

int yn_op_f32_maxpool(yn_handle* h, const float* x, int B, int H, int W, int C, float* y, int32_t* idx, const float* dy, float* dx)
{
    YN_ENTER(h);
    if (!x || !y || !idx || B <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(h, "yn_op_f32_maxpool: bad arguments");
    if (!dy != !dx) return fail(h, "yn_op_f32_maxpool: dy and dx come together");
    if (dy && (C & 1)) return fail(h, "yn_op_f32_maxpool: the backward kernel needs an even C");
    launch_maxpool_idx(x, B, H, W, C, y, idx, h->stream);
    if (dy) launch_maxpool_bwd(dy, idx, B, H, W, C, dx, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_op_f32_resample(yn_handle* h, int mode, const float* a, const float* b, float* out, int B, int H, int W, int C)
{
    YN_ENTER(h);
    if (mode < 0 || mode > 3 || !a || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(h, "yn_op_f32_resample: bad arguments");
    if (mode <= 1 && !b) return fail(h, "yn_op_f32_resample: modes 0 and 1 add two tensors");
    if ((mode == 0 || mode == 2) && ((H | W) & 1)) return fail(h, "yn_op_f32_resample: the high-resolution map of modes 0 and 2 has an even extent");
    launch_resample(a, b, out, B, H, W, C, mode, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
