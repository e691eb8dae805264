// yn_train_api.inc — the training step's entry points, included by yn_api.hip last: the per-precision step functions around train_tape
// (yn_train_tape.inc) and the extern "C" surface of training.

namespace {

int train_step_f32(yn_handle* h, const float* x_dev, const float* target_dev, int B, float lr, float momentum, float weight_decay,
                   float grad_scale, int do_update, float* losses_dev)
{
    hipStream_t st = h->stream;
    h->cur = st;
    if (ensure_train_arena(h, B, h->grid.S, 10)) return 1;
    Trainer T(h, B, read_train_switches());
    if (h->multi_stream && !h->profiling) {
        if (!h->side[0] && hipStreamCreateWithFlags(&h->side[0], hipStreamNonBlocking) != hipSuccess) h->side[0] = nullptr;
        if (h->side[0]) {
            if (ensure_train_events(h, (size_t)NEV + 1)) return 1;
            T.sq.attach(h, h->side[0]);
        }
    }
    if (T.begin()) return 1;
    if (train_tape(T, x_dev, target_dev, losses_dev)) return 1;
    if (h->fwd_only[0]) return 0;
    if (do_update && optimiser_tail(h, lr, momentum, weight_decay, grad_scale, st)) return 1;
    h->folded = false;                                    // inference packs are stale now
    return 0;
}

// Everything of the fp16 step between the host-side preparation and the optimiser: loss-scale settlement, weight packs, forward, loss, backward,
// gradient combine.  No allocation, no synchronisation, the same launches with the same arguments for the same (x, target, losses, B, S, switches):
// the part train_step_h16 captures into a hipGraph.
int train_body_h16(yn_handle* h, const float* x_dev, const float* target_dev, int B, float* losses_dev, const TrainSwitches& sw)
{
    launch_hscale_update(h->scale_state, nullptr, h->stream);     // a previous step nobody ran yn_sgd_step for: settle its scale decision from the local flag
    HTrainer T(h, B, sw);
    if (T.begin()) return 1;
    return train_tape(T, x_dev, target_dev, losses_dev);
}

int train_step_h16(yn_handle* h, const float* x_dev, const float* target_dev, int B, float lr, float momentum, float weight_decay,
                   float grad_scale, int do_update, float* losses_dev)
{
    const int S = h->grid.S;
    hipStream_t st = h->stream;
    h->cur = st;
    // ---- host-side preparation: everything that allocates or synchronises ----
    const TrainSwitches sw = read_train_switches();
    if (ensure_train_arena(h, B, S, 7)) return 1;                                      // fp16 tensors, padded channels
    if (h->hpacks.empty()) h->hpacks.resize(h->layers.size());
    if (!h->scale_state) {
        HIPCHK(h, h->scale_state.reserve(8));
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
        if (h->train_side && ensure_train_events(h, (size_t)NEV + 9)) return 1;
    }
    if (ensure_loss(h, B)) return 1;
    HIPCHK(h, h->train_losses.reserve(4));

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
    const bool graphable = h->train_graph && st != nullptr && !h->profiling && !h->fwd_only[0] && !sw.poison && h->train_graph_misses < 64;
    int rc = 0;
    bool ran = false;
    if (graphable) {
        // the per-step test switches select different launches (and a different arena carve): part of the key, or a flipped switch replays the stale form
        const std::vector<uintptr_t> key{(uintptr_t)x_dev, (uintptr_t)target_dev, (uintptr_t)B, (uintptr_t)S, (uintptr_t)h->multi_stream, (uintptr_t)h->head_fork_now, sw.key()};
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
            rc = train_body_h16(h, x_dev, target_dev, B, h->train_losses, sw);
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
        rc = train_body_h16(h, x_dev, target_dev, B, h->train_losses, sw);
        if (rc) return rc;
    }
    if (trial >= 0) HIPCHK(h, hipEventRecord(h->fork_ev[2 * trial + 1], st));
    if (h->fwd_only[0]) return 0;
    if (losses_dev) HIPCHK(h, hipMemcpyAsync(losses_dev, h->train_losses, 4 * sizeof(float), hipMemcpyDeviceToDevice, st));

    if (do_update && optimiser_tail(h, lr, momentum, weight_decay, grad_scale, st)) return 1;
    h->folded = false;
    return 0;
}
}  // namespace

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
    if (h->hpack_table) { HIPCHK(h, hipStreamSynchronize(h->stream)); h->hpack_table.reset(); }
    h->hpack_jobs.clear();                                 // the fp16 step's pack table points into the (new) flat parameter buffer
    if (zeros_ready(h)) return 1;
    // per-layer packs (forward: raw weights; backward: transposed / flipped)
    if (h->tpacks.empty()) {
        h->tpacks.resize(h->layers.size());
        for (size_t i = 0; i < h->layers.size(); ++i)
            if (alloc_packs(h, h->layers[i], h->tpacks[i])) return 1;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int yn_train_step(yn_handle* h, const float* x_dev, const float* target_dev, int B, float lr, float momentum, float weight_decay,
                  float grad_scale, int do_update, float* losses_dev)
{
    YN_ENTER(h);
    if (need_square_grid(h, "yn_train_step")) return 1;
    if (!h->tP) return fail(h, "yn_train_step before yn_train_bind");
    if (B <= 0) return fail(h, "batch must be positive (got %d)", B);
    return (h->train_dtype == YN_F16 ? train_step_h16 : train_step_f32)(h, x_dev, target_dev, B, lr, momentum, weight_decay, grad_scale, do_update, losses_dev);
}

int yn_train_forward(yn_handle* h, const float* x_dev, int B, float* head_s8, float* head_s16, float* head_s32)
{
    YN_ENTER(h);
    if (need_square_grid(h, "yn_train_forward")) return 1;
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
    if (dtype == YN_F16) {
        // the fp16 step's reducing and BatchNorm kernels (hcol_reduce_kernel, hdw_wgrad_kernel, hbn_apply_kernel, hbn_bwd_kernel) combine at most 32
        // octet lanes and keep 256 channel constants in LDS: a layer above 256 padded channels (bf = 352 / 488 of the 1.5x / 2.0x backbones) is refused
        // here, not computed wrongly.  A depthwise conv may read a two-plane unit tensor: 2 * roundup8(C / 2) physical channels.
        for (const Layer& l : h->layers) {
            if (l.kind == K_STEM || (l.bn.empty() && l.kind != K_DW && !l.has_bias)) continue;
            const int Cp = l.kind == K_DW ? 2 * r8((l.cout + 1) / 2) : r8(l.cout);
            if (Cp > 256) return fail(h, "yn_train_precision: the fp16 step serves layers of at most 256 padded channels; %s has %d (the 0.5x and 1.0x backbones fit, 1.5x and 2.0x train in fp32)", l.name.c_str(), l.cout);
        }
    }
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
