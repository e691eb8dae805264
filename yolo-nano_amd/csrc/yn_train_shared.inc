// yn_train_shared.inc — what the two executors of the training step (yn_train.inc: fp32, yn_train_h16.inc: fp16) have in common,
// included by yn_api.hip before both: the per-step test switches, the step arena, the fixed scratch, the side queue of the weight
// gradients, arena growth, the optimiser tail and the flat parameter order.

namespace {

// The per-step test switches, parsed HERE and nowhere else: the executor flags, the stem choice, `graphable` and the graph key all read this
// struct, so they cannot disagree.  Read at every step, not once per process: the tests compare the two forms of a step inside one process.
struct TrainSwitches {
    bool fuse_stats, fuse_sums;         // fp16: HColStat epilogues (0: separate reduction launches)
    bool stem_fuse;                     // fp16: the stem's BatchNorm + activation + max pool as one kernel (0: the separate launches)
    bool poison;                        // NaN-fill the activation-gradient region before the loss
    uintptr_t key() const { return (uintptr_t)fuse_stats | (uintptr_t)fuse_sums << 1 | (uintptr_t)stem_fuse << 2; }   // they select different launches (and a different arena carve)
};
inline bool switch_on(const char* v, bool dflt) { return v ? atoi(v) != 0 : dflt; }
TrainSwitches read_train_switches()
{
    return TrainSwitches{switch_on(getenv("YN_TRAIN_FUSE_STATS"), true), switch_on(getenv("YN_TRAIN_FUSE_SUMS"), true),
                         switch_on(getenv("YN_TRAIN_STEM_FUSE"), true), switch_on(getenv("YN_TRAIN_POISON"), false)};
}

// One step's workspace: values grow up from the start, gradient tensors grow down from the end (one contiguous region: the poison hook
// fills it with one memset).  Nothing is reused within a step.  Exhaustion latches `oom` and hands out the base: checked once, after the forward.
struct StepArena {
    char* base; size_t cap;
    size_t used = 0, gused = 0;
    bool oom = false;
    bool fits(size_t& bytes) { bytes = (bytes + 255) & ~(size_t)255; if (used + bytes + gused > cap) oom = true; return used + bytes + gused <= cap; }
    void* up(size_t bytes) { if (!fits(bytes)) return base; void* p = base + used; used += bytes; return p; }
    void* down(size_t bytes) { if (!fits(bytes)) return base; gused += bytes; return base + cap - gused; }
    char* grads() const { return base + cap - gused; }
};

// The fixed fp32 scratch of a step: BatchNorm sum accumulators (one memset per step), the per-slice weight-gradient copies of one layer at
// a time, GRAD_SLOTS copies of the flat gradient buffer (atomics targets; slot s is h->tN floats further).
constexpr size_t WPART_FLOATS = (size_t)16 << 20;       // floats of weight-gradient scratch
struct StepScratch {
    double* stats = nullptr; size_t stats_used = 0, stats_cap = 0;
    float* wpart = nullptr; size_t wpart_cap = 0;
    float* gslots = nullptr;
    double* take_stats(size_t n) { if (stats_used + n > stats_cap) return nullptr; double* p = stats + stats_used; stats_used += n; return p; }
};
// carve it (acc_slots accumulator copies per BatchNorm channel) and zero what accumulates, the flat gradient buffer included
int carve_scratch(yn_handle* h, StepArena& ar, int acc_slots, hipStream_t st, StepScratch& sc)
{
    size_t nstat = 0;
    for (const Layer& l : h->layers) if (!l.bn.empty()) nstat += 4 * acc_slots * (size_t)l.cout;
    sc.stats = (double*)ar.up(nstat * sizeof(double));
    sc.stats_cap = nstat;
    HIPCHK(h, hipMemsetAsync(sc.stats, 0, nstat * sizeof(double), st));
    sc.wpart_cap = WPART_FLOATS;
    sc.wpart = (float*)ar.up(sc.wpart_cap * sizeof(float));
    sc.gslots = (float*)ar.up((size_t)GRAD_SLOTS * h->tN * sizeof(float));
    HIPCHK(h, hipMemsetAsync(sc.gslots, 0, (size_t)GRAD_SLOTS * h->tN * sizeof(float), st));
    HIPCHK(h, hipMemsetAsync(h->tG, 0, h->tN * sizeof(float), st));
    return 0;
}

// What both executors carry: the handle, the step's geometry, the stream launches go to, the switches, the workspace, one record per layer run.
template <class Rec> struct StepBase {
    yn_handle* h;
    int B, S;
    hipStream_t st;                                         // the main stream, or a head tower's while the tape issues that tower
    TrainSwitches sw;
    StepArena ar;
    StepScratch sc;
    std::vector<Rec> recs;
    StepBase(yn_handle* h_, int B_, const TrainSwitches& sw_) : h(h_), B(B_), S(h_->grid.S), st(h_->stream), sw(sw_), ar{h_->train_arena, h_->train_arena.cap()} { recs.reserve(h->layers.size() + 4); }
    float* P(const std::string& k) { return h->tP + h->toff.at(k); }
    float* G(const std::string& k) { return h->tG + h->toff.at(k); }
    float* GS(const std::string& k) { return sc.gslots + h->toff.at(k); }   // slot 0; slot s is h->tN floats further
};

// Weight gradients run on a side stream, concurrently with the BatchNorm-backward / input-gradient chain on the main stream: they only
// depend on dy (and the saved activations) and nothing but the optimiser waits for them.  A layer's BatchNorm backward writes dy IN PLACE
// over the pre-BN conv output y (nothing reads y afterwards), so no buffer is reused and the side stream only ever waits for the main one:
// one event per BATCH layers (an event record costs the main queue ~7 us of idle time before its next kernel: 1.2 ms per step with one
// per layer).  P is the executor's record of one pending layer, `run` launches its weight gradients.
constexpr int NEV = 32, BATCH = 4;                      // events the hand-over cycles through; layers per hand-over
template <class P> struct SideQueue {
    hipStream_t side = nullptr;
    hipEvent_t ev[NEV];
    int ei = 0;
    std::vector<P> pending;
    hipStream_t fk[2] = {nullptr, nullptr};                 // fp16, when the head towers fork: the streams of towers 3 / 4, and their events
    hipEvent_t fev[8];

    void attach(yn_handle* h, hipStream_t s) { side = s; for (int i = 0; i < NEV; ++i) ev[i] = h->train_events[i]; }
    template <class F> void add(hipStream_t st, const P& p, F&& run)
    {
        if (!side) { run(p); return; }
        pending.push_back(p);
        if ((int)pending.size() >= BATCH) flush(st, run);
    }
    // everything queued so far is complete on `st` after this point: hand it to the side stream
    template <class F> void flush(hipStream_t st, F&& run)
    {
        if (pending.empty()) return;
        hipEvent_t e = ev[ei++ % NEV];
        (void)hipEventRecord(e, st);
        (void)hipStreamWaitEvent(side, e, 0);
        for (const P& p : pending) run(p);
        pending.clear();
    }
    // every weight gradient is in before the slots are combined on `st`
    int join(yn_handle* h, hipStream_t st)
    {
        if (!side) return 0;
        hipEvent_t e = h->train_events[NEV];
        HIPCHK(h, hipEventRecord(e, side));
        HIPCHK(h, hipStreamWaitEvent(st, e, 0));
        return 0;
    }
};

int ensure_train_events(yn_handle* h, size_t n)
{
    while (h->train_events.size() < n) {
        hipEvent_t e;
        HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->train_events.push_back(e);
    }
    return 0;
}

// activations + gradients (`factor` times the inference arena), plus the fixed scratch (weight-gradient slices, gradient slots, BN sums)
int ensure_train_arena(yn_handle* h, int B, int S, int factor)
{
    const size_t need = network_arena_bytes(h, B, S) * factor + ((size_t)256 << 20);
    if (need <= h->train_arena.cap()) return 0;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    drop_train_graphs(h);                                   // captured steps bake the arena's addresses in
    HIPCHK(h, h->train_arena.reserve(need));
    return 0;
}

// optimizer.step() behind the step; the fp16 step's loss scale follows the same finite-scan
int optimiser_tail(yn_handle* h, float lr, float momentum, float weight_decay, float grad_scale, hipStream_t st)
{
    if (!h->skip_flag) {
        HIPCHK(h, h->skip_flag.reserve(2));
        HIPCHK(h, hipMemsetAsync(h->skip_flag, 0, 2 * sizeof(int), st));
    }
    launch_sgd(h->tP, h->tG, h->tM, (long)h->tN, lr, momentum, weight_decay, grad_scale, 0, h->skip_flag, st);   // momentum starts at zero: no first-step case
    if (h->train_dtype == YN_F16) launch_hscale_update(h->scale_state, h->skip_flag, st);
    h->train_steps++;
    HIPCHK(h, hipGetLastError());
    return 0;
}

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
