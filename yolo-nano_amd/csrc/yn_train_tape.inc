// yn_train_tape.inc — the training step's network wiring, ONCE for both precisions, included by yn_api.hip after the two executors
// (yn_train.inc: Trainer, fp32; yn_train_h16.inc: HTrainer, fp16).  models/yolo_nano.py:282-358 and backbone/shufflenetv2.py:69-78
// forward, the loss, then the same in reverse with the "first writer / accumulate" decisions.  What one layer does in a precision is
// the executor X's business; the tape asks it for
//   tensors   mk(M, C), mk_unit(M, bf) (a ShuffleV2 unit's output), mk_like(t, M) (t's channel map at another M), out_of(rec, g);
//   views     full(t, grad), plane(unit, 0 | 1, grad);
//   forward   stem_fwd, conv -> record index, bn, bn_shuffle, resample, forward_done, loss;
//   backward  back(rec, dz, dx, accumulate, need_input, below), back_unit_s1 / back_unit_s2 / even_to (a unit's output gradient splits
//             into pw2's backward from the odd channels and the pass-through even half: each precision orders the two its own way),
//             stem_bwd, flush_params, combine;
//   streams   st (where launches go), sq.fk[k] (the stream of head tower k, null when towers do not fork: always in fp32).

namespace {

template <class X>
int train_tape(X& T, const float* x_dev, const float* target_dev, float* losses_dev)
{
    using Ten = typename X::Ten;
    yn_handle* h = T.h;
    const int B = T.B, S = T.S;
    const hipStream_t st = T.st;                            // the main stream (T.st moves to a tower's stream while that tower is issued)

    // =============================== forward (train mode) ===============================
    const Ten a1 = T.stem_fwd(x_dev);                       // stem conv + BN + act + 3x3 / 2 max pool
    struct Blk { int s2; int r_b1dw, r_b1pw, r_pw1, r_dw, r_pw2; Ten in, tdw1, tb1, t1, t2, out; };
    std::vector<Blk> blks;
    Ten cur = a1;
    int curH = S / 4;
    Ten cfeat[3];
    char nm[96];
    for (int si = 0; si < 3; ++si) {
        const int bf = h->stage_ch[si] / 2;
        for (int bi = 0; bi < STAGE_REP[si]; ++bi) {
            snprintf(nm, sizeof nm, "backbone.stage%d.%d", si + 2, bi);
            const std::string Pn = nm;
            Blk k{};
            k.in = cur;
            if (bi == 0) {
                const int Ho = curH / 2;
                const long Mi = (long)B * curH * curH, Mo = (long)B * Ho * Ho;
                k.s2 = 1;
                k.tdw1 = T.mk_like(cur, Mo); k.tb1 = T.mk(Mo, bf); k.t1 = T.mk(Mi, bf); k.t2 = T.mk(Mo, bf); k.out = T.mk_unit(Mo, bf);
                k.r_b1dw = T.conv(L(h, Pn + ".b1.dw"), X::full(cur), B, curH, curH); T.bn(k.r_b1dw, k.tdw1);
                k.r_b1pw = T.conv(L(h, Pn + ".b1.pw"), X::full(k.tdw1), B, Ho, Ho); T.bn(k.r_b1pw, k.tb1);
                k.r_pw1 = T.conv(L(h, Pn + ".b2.pw1"), X::full(cur), B, curH, curH); T.bn(k.r_pw1, k.t1);
                k.r_dw = T.conv(L(h, Pn + ".b2.dw"), X::full(k.t1), B, curH, curH); T.bn(k.r_dw, k.t2);
                k.r_pw2 = T.conv(L(h, Pn + ".b2.pw2"), X::full(k.t2), B, Ho, Ho);
                T.bn_shuffle(k.r_pw2, X::full(k.tb1), k.out);                                      // out[2j] = b1[j], out[2j+1] = b2[j]
                curH = Ho;
            } else {
                const long Mo = (long)B * curH * curH;
                k.s2 = 0;
                k.t1 = T.mk(Mo, bf); k.t2 = T.mk(Mo, bf); k.out = T.mk_unit(Mo, bf);
                k.r_pw1 = T.conv(L(h, Pn + ".b2.pw1"), X::plane(cur, 1), B, curH, curH); T.bn(k.r_pw1, k.t1);
                k.r_dw = T.conv(L(h, Pn + ".b2.dw"), X::full(k.t1), B, curH, curH); T.bn(k.r_dw, k.t2);
                k.r_pw2 = T.conv(L(h, Pn + ".b2.pw2"), X::full(k.t2), B, curH, curH);
                T.bn_shuffle(k.r_pw2, X::plane(cur, 0), k.out);                                    // out[2j] = x1[j]
            }
            cur = k.out;
            blks.push_back(k);
        }
        cfeat[si] = cur;
    }
    // neck
    const int W3 = S / 8, W4 = S / 16, W5 = S / 32;
    const long M3 = (long)B * W3 * W3, M4 = (long)B * W4 * W4, M5 = (long)B * W5 * W5;
    Ten p3 = T.mk(M3, NECK), p4 = T.mk(M4, NECK), p5 = T.mk(M5, NECK);
    Ten u4 = T.mk(M4, NECK), p4a = T.mk(M4, NECK), u3 = T.mk(M3, NECK), p3a = T.mk(M3, NECK), d4 = T.mk(M4, NECK), p4b = T.mk(M4, NECK), d5 = T.mk(M5, NECK), p5a = T.mk(M5, NECK);
    // u = p + up2(q) / d = p + down(q): the gradient of the sum IS the gradient of its same-resolution term, so the two share one buffer
    // (the sum's gradient has been consumed by the time the term's other contributions are accumulated into it): four device copies less
    p5.g = d5.g; p4a.g = d4.g; p3.g = u3.g; p4.g = u4.g;
    const int r_lat0 = T.conv(L(h, "conv1x1_0"), X::full(cfeat[0]), B, W3, W3); T.bn(r_lat0, p3);
    const int r_lat1 = T.conv(L(h, "conv1x1_1"), X::full(cfeat[1]), B, W4, W4); T.bn(r_lat1, p4);
    const int r_lat2 = T.conv(L(h, "conv1x1_2"), X::full(cfeat[2]), B, W5, W5); T.bn(r_lat2, p5);
    T.resample(p4.v, p5.v, u4.v, W4, 0);
    const int r_sm0 = T.conv(L(h, "smooth_0"), X::full(u4), B, W4, W4); T.bn(r_sm0, p4a);
    // The three head towers are independent chains of small kernels (19x19 / 38x38 maps: 6-10 us launches that fill a fraction of the chip):
    // when they fork, level 3 starts on a stream of its own as soon as smooth_1 is done and runs beside the rest of the neck, level 4 on a
    // second one, level 5 stays on the main stream; all join before the loss.  (Backward: the same towers fork again after the loss.)
    const Ten feats[3] = {p3a, p4b, p5a};
    const int Ws[3] = {W3, W4, W5};
    struct HeadT { Ten t[4]; int r[5]; };
    HeadT hd[3];
    Ten raw[3];                                                                                   // the raw heads [M][HCp] and their gradients
    // the three raw-head gradients in ONE block (one memset before the loss instead of three)
    const int HCp = X::head_ld(h->head_ch);
    const size_t gout_off[3] = {0, (size_t)M3 * HCp, (size_t)(M3 + M4) * HCp};
    const size_t gout_total = (size_t)(M3 + M4 + M5) * HCp;
    auto* gout_all = T.take_g(gout_total);
    hipStream_t* fk = T.sq.fk;
    hipEvent_t* fev = T.sq.fev;
    auto head_fwd = [&](int k, hipStream_t on) {
        if (on) { (void)hipEventRecord(fev[k], st); (void)hipStreamWaitEvent(on, fev[k], 0); T.st = on; }
        const long M = (long)B * Ws[k] * Ws[k];
        snprintf(nm, sizeof nm, "head_det_%d", k + 1);
        const std::string Pn = nm;
        for (int j = 0; j < 4; ++j) hd[k].t[j] = T.mk(M, NECK);
        Ten in = feats[k];
        for (int j = 0; j < 4; ++j) {
            hd[k].r[j] = T.conv(L(h, Pn + "." + std::to_string(j)), X::full(in), B, Ws[k], Ws[k]);
            T.bn(hd[k].r[j], hd[k].t[j]);
            in = hd[k].t[j];
        }
        hd[k].r[4] = T.conv(L(h, Pn + ".4"), X::full(in), B, Ws[k], Ws[k]);       // plain conv + bias, no BN: its output IS the raw head
        raw[k] = T.out_of(hd[k].r[4], gout_all + gout_off[k]);
        T.st = st;
    };
    T.resample(p3.v, p4a.v, u3.v, W3, 0);
    const int r_sm1 = T.conv(L(h, "smooth_1"), X::full(u3), B, W3, W3); T.bn(r_sm1, p3a);
    T.resample(p4a.v, p3a.v, d4.v, W4, 1);
    head_fwd(0, fk[0]);                                                          // (after the resample that also reads p3a: one event covers both)
    const int r_sm2 = T.conv(L(h, "smooth_2"), X::full(d4), B, W4, W4); T.bn(r_sm2, p4b);
    T.resample(p5.v, p4b.v, d5.v, W5, 1);
    head_fwd(1, fk[1]);
    const int r_sm3 = T.conv(L(h, "smooth_3"), X::full(d5), B, W5, W5); T.bn(r_sm3, p5a);
    head_fwd(2, nullptr);
    for (int i = 0; i < 2; ++i)
        if (fk[i]) { (void)hipEventRecord(fev[2 + i], fk[i]); (void)hipStreamWaitEvent(st, fev[2 + i], 0); }
    if (T.ar.oom) return fail(h, "training workspace exhausted (%zu bytes)", h->train_arena.cap());
    if (T.forward_done()) return 1;
    if (h->fwd_only[0]) {                                  // yn_train_forward: raw heads as dense fp32 rows, nothing else
        for (int k = 0; k < 3; ++k) launch_rows_to_f32(raw[k].v, X::is_h16, HCp, h->fwd_only[k], h->head_ch, raw[k].M, st);
        HIPCHK(h, hipGetLastError());
        return 0;
    }

    // =============================== loss (+ gradient w.r.t. the raw heads) ===============================
    if (ensure_loss(h, B)) return 1;
    // Only the head gradients need zeros (the loss kernel writes the positives' class gradients only, and the pad column).
    // Every activation gradient below is fully written by its FIRST producer (a plain store) before anything
    // accumulates into it — see the first-writer notes at each call — so the region is never memset.
    if (T.sw.poison) HIPCHK(h, hipMemsetAsync(T.ar.grads(), 0xff, T.ar.gused, st));                // test hook: NaN-fill the gradient region first
    HIPCHK(h, hipMemsetAsync(gout_all, 0, gout_total * sizeof(*gout_all), st));
    T.loss(raw, target_dev, losses_dev);

    // =============================== backward ===============================
    // heads: every head accumulates into the gradient of its pyramid level
    auto head_bwd = [&](int k, hipStream_t on) {
        if (on) { T.flush_params(); T.st = on; }                                           // (queued weight gradients belong to the stream they were queued on)
        T.back(hd[k].r[4], X::full(raw[k], true), X::full(hd[k].t[3], true), false, true, hd[k].r[3]);
        for (int j = 3; j >= 1; --j) T.back(hd[k].r[j], X::full(hd[k].t[j], true), X::full(hd[k].t[j - 1], true), false, true, hd[k].r[j - 1]);
        T.back(hd[k].r[0], X::full(hd[k].t[0], true), X::full(feats[k], true), false);     // first writer of p3a / p4b / p5a
        if (on) { T.flush_params(); (void)hipEventRecord(fev[5 + k], on); T.st = st; }
    };
    if (fk[0]) {
        (void)hipEventRecord(fev[4], st);                                                  // the loss is done: the towers' backward passes fork
        (void)hipStreamWaitEvent(fk[0], fev[4], 0); (void)hipStreamWaitEvent(fk[1], fev[4], 0);
    }
    head_bwd(0, fk[0]);
    head_bwd(1, fk[1]);
    head_bwd(2, nullptr);                                                                  // level 5 on the main stream: the neck's backward needs it first
    // PAN / FPN (models/yolo_nano.py:291-296), in reverse
    T.back(r_sm3, X::full(p5a, true), X::full(d5, true), false);                           // d5.g IS p5.g (d5 = p5 + down(p4b))
    if (fk[1]) (void)hipStreamWaitEvent(st, fev[6], 0);                                    // level 4's tower has written p4b.g
    T.resample(d5.g, nullptr, p4b.g, W5, 3);
    T.back(r_sm2, X::full(p4b, true), X::full(d4, true), false);
    if (fk[0]) (void)hipStreamWaitEvent(st, fev[5], 0);                                    // level 3's tower has written p3a.g
    T.resample(d4.g, nullptr, p3a.g, W4, 3);
    T.back(r_sm1, X::full(p3a, true), X::full(u3, true), false);
    T.resample(u3.g, nullptr, p4a.g, W3, 2);
    T.back(r_sm0, X::full(p4a, true), X::full(u4, true), false);
    T.resample(u4.g, nullptr, p5.g, W4, 2);
    T.back(r_lat2, X::full(p5, true), X::full(cfeat[2], true), false);                     // laterals: first writers of the stage outputs' gradients
    T.back(r_lat1, X::full(p4, true), X::full(cfeat[1], true), false);
    T.back(r_lat0, X::full(p3, true), X::full(cfeat[0], true), false);
    // backbone blocks in reverse (backbone/shufflenetv2.py:69-78): out[2j] = the pass-through (x1 / branch1), out[2j+1] = branch2[j]
    for (int bi = (int)blks.size() - 1; bi >= 0; --bi) {
        Blk& k = blks[bi];
        if (!k.s2) {
            // k.in is never a stage output: its gradient is written once, plane 0 by the pass-through half and plane 1 by pw1's input gradient
            T.back_unit_s1(k.r_pw2, k.out, X::full(k.t2, true), X::plane(k.in, 0, true), k.r_dw);
            T.back(k.r_dw, X::full(k.t2, true), X::full(k.t1, true), false, true, k.r_pw1);
            T.back(k.r_pw1, X::full(k.t1, true), X::plane(k.in, 1, true), false);
        } else {
            const bool b1_done = T.back_unit_s2(k.r_pw2, k.out, X::full(k.t2, true), X::full(k.tb1, true), k.r_dw);
            T.back(k.r_dw, X::full(k.t2, true), X::full(k.t1, true), false, true, k.r_pw1);
            // k.in is the previous stage's output (its lateral wrote the gradient first) or the max-pool output (nobody did)
            T.back(k.r_pw1, X::full(k.t1, true), X::full(k.in, true), k.in.g != a1.g);
            if (!b1_done) T.even_to(k.out, X::full(k.tb1, true));                          // gradient of branch1's output
            T.back(k.r_b1pw, X::full(k.tb1, true), X::full(k.tdw1, true), false, true, k.r_b1dw);
            T.back(k.r_b1dw, X::full(k.tdw1, true), X::full(k.in, true), true);
        }
    }
    T.stem_bwd();                                                                          // max pool + stem
    T.flush_params();
    if (T.sq.join(h, st)) return 1;
    T.combine();
    HIPCHK(h, hipGetLastError());
    return 0;
}

}  // namespace
