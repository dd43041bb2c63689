// runtime.hip — error text, device info, the static-program executor and hipGraph capture/replay.
//
// The reference drives its network through Python autograd, one torch operator at a time
// (models.py:105-136).  Here a step is a flat, static list of operator descriptors built once by the
// host; running it is ONE call that enqueues every kernel on a HIP stream, and the same list can be
// captured into a hipGraph so that a launch-bound step costs one graph launch.
#include <stdarg.h>
#include <string.h>
#include <stdlib.h>
#include "common.h"

static thread_local char g_err[512] = "";

void salt_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* salt_last_error(void) { return g_err; }

extern "C" int salt_abi_version(void) { return 34; }

extern "C" int salt_device_info(int* cu_count, int* lds_bytes, char* arch_name, int arch_name_len) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) SALT_FAIL((int)e, "hipGetDevice: %s", hipGetErrorString(e));
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, dev);
    if (e != hipSuccess) SALT_FAIL((int)e, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (cu_count) *cu_count = prop.multiProcessorCount;
    if (lds_bytes) *lds_bytes = (int)prop.sharedMemPerBlock;
    if (arch_name && arch_name_len > 0) { strncpy(arch_name, prop.gcnArchName, arch_name_len - 1); arch_name[arch_name_len - 1] = 0; }
    return SALT_OK;
}

extern "C" int salt_program_run_range(const salt_program_entry* e, int begin, int end, void* stream) {
    if (!e || begin < 0 || end < begin) SALT_FAIL(SALT_E_BADARG, "program: bad range");
    for (int i = begin; i < end; ++i) {
        const int rc = e[i].fn(e[i].args, stream);
        if (rc) {
            char prev[400];
            strncpy(prev, g_err, sizeof(prev) - 1); prev[sizeof(prev) - 1] = 0;
            salt_set_error("program entry %d failed (%d): %s", i, rc, prev);
            return rc;
        }
    }
    return SALT_OK;
}

// Same as salt_program_run_range but brackets every entry with HIP events recorded on `stream` (the stream the
// kernels are launched on) and returns the elapsed milliseconds per entry.  Used by bench.py for the live roofline.
extern "C" int salt_program_run_timed(const salt_program_entry* e, int begin, int end, void* stream, float* ms_out) {
    if (!e || begin < 0 || end < begin || !ms_out) SALT_FAIL(SALT_E_BADARG, "program: bad range");
    const int n = end - begin;
    hipStream_t st = (hipStream_t)stream;
    hipEvent_t* ev = new hipEvent_t[n + 1];
    for (int i = 0; i <= n; ++i) if (hipEventCreate(&ev[i]) != hipSuccess) { delete[] ev; SALT_FAIL(SALT_E_BADARG, "hipEventCreate failed"); }
    int rc = SALT_OK;
    (void)hipEventRecord(ev[0], st);
    for (int i = 0; i < n && rc == SALT_OK; ++i) {
        rc = e[begin + i].fn(e[begin + i].args, stream);
        (void)hipEventRecord(ev[i + 1], st);
    }
    (void)hipStreamSynchronize(st);
    if (rc == SALT_OK) for (int i = 0; i < n; ++i) { float ms = 0.f; (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]); ms_out[i] = ms; }
    for (int i = 0; i <= n; ++i) (void)hipEventDestroy(ev[i]);
    delete[] ev;
    return rc;
}

namespace {
// The fork / join events only order two streams of ONE device.  Default events: creating them with hipEventDisableSystemFence or
// hipEventReleaseToDevice (device-scope release instead of the system-scope fence) had no measurable effect on the step.
constexpr unsigned kForkEventFlags = hipEventDisableTiming;
struct EventPool {
    hipEvent_t ev[2] = {nullptr, nullptr};
    int ensure() {
        for (int i = 0; i < 2; ++i)
            if (!ev[i] && hipEventCreateWithFlags(&ev[i], kForkEventFlags) != hipSuccess) return -1;
        return 0;
    }
};
thread_local EventPool g_events;
thread_local hipEvent_t g_fork_event = nullptr;
thread_local bool g_capturing = false;         // the stop event of a salt_launch_ev launch is not capturable: plain event forks while a graph records
// Side-stream entries are issued behind one fork per this many groups.  Eager run: 1, a fork per layer that rides on the producing
// kernel's completion signal (6.18 ms per step; explicit event record 6.25, one fork per two layers 6.30).  While a hipGraph is captured: 8 (a
// cross-stream edge of a replayed graph stalls the main branch ~10 us, a live event does not).
constexpr int kForkEveryEager = 1, kForkEveryGraph = 8;
}  // namespace

hipEvent_t salt_take_fork_event() { hipEvent_t e = g_fork_event; g_fork_event = nullptr; return e; }

extern "C" int salt_program_run_streams(const salt_program_entry* e, int begin, int end, void* main_stream, void* side_stream) {
    return salt_program_run_streams_ex(e, begin, end, main_stream, side_stream, 1);
}

extern "C" int salt_program_run_streams_ex(const salt_program_entry* e, int begin, int end, void* main_stream, void* side_stream, int join_at_end) {
    return salt_program_run_streams_marks(e, begin, end, main_stream, side_stream, join_at_end, nullptr, 0, nullptr, nullptr);
}

extern "C" int salt_event_create(void** out) {
    if (!out) SALT_FAIL(SALT_E_BADARG, "event_create: null");
    hipEvent_t ev = nullptr;
    const hipError_t err = hipEventCreateWithFlags(&ev, kForkEventFlags);
    if (err != hipSuccess) SALT_FAIL((int)err, "hipEventCreate: %s", hipGetErrorString(err));
    *out = ev;
    return SALT_OK;
}
extern "C" int salt_event_destroy(void* ev) { if (ev) (void)hipEventDestroy((hipEvent_t)ev); return SALT_OK; }
extern "C" int salt_stream_wait_event(void* stream, void* ev) {
    if (!ev) SALT_FAIL(SALT_E_BADARG, "stream_wait_event: null event");
    const hipError_t err = hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)ev, 0);
    if (err != hipSuccess) SALT_FAIL((int)err, "hipStreamWaitEvent: %s", hipGetErrorString(err));
    return SALT_OK;
}

extern "C" int salt_program_run_streams_marks(const salt_program_entry* e, int begin, int end, void* main_stream, void* side_stream, int join_at_end,
                                              const int* marks, int nmarks, void* const* ev_main, void* const* ev_side) {
    if (nmarks < 0 || (nmarks > 0 && (!marks || !ev_main || !ev_side))) SALT_FAIL(SALT_E_BADARG, "program: marks");
    if (!side_stream || side_stream == main_stream) {
        if (nmarks) SALT_FAIL(SALT_E_BADARG, "program: marks need the two-stream executor");
        return salt_program_run_range(e, begin, end, main_stream);
    }
    if (!e || begin < 0 || end < begin) SALT_FAIL(SALT_E_BADARG, "program: bad range");
    if (g_events.ensure()) SALT_FAIL(SALT_E_BADARG, "hipEventCreate failed");
    hipStream_t ms = (hipStream_t)main_stream, ss = (hipStream_t)side_stream;
    bool main_dirty = true, side_used = false;       // main_dirty: main has work the side stream has not been ordered after
    // Fork coalescing (fork_every = K > 1): side-stream entries are held back until K groups of them are pending, then issued
    // behind ONE fork.  A held entry only ever runs later than its program position, so its inputs are complete; every cross-queue
    // dependency costs the main queue ~10 us of dispatch stall (rocprofv3 timeline), a held entry costs the side stream its head start.
    const int fork_every = g_capturing ? kForkEveryGraph : kForkEveryEager;
    int pending[64], npending = 0, groups = 0;
    bool prev_side = false;
    auto flush = [&]() -> int {
        if (!npending) return 0;
        if (main_dirty) {
            (void)hipEventRecord(g_events.ev[0], ms);
            (void)hipStreamWaitEvent(ss, g_events.ev[0], 0);
            main_dirty = false;
        }
        for (int k = 0; k < npending; ++k) {
            const int j = pending[k];
            const int rc = e[j].fn(e[j].args, side_stream);
            if (rc) { char prev[400]; strncpy(prev, g_err, sizeof(prev) - 1); prev[sizeof(prev) - 1] = 0; salt_set_error("program entry %d failed (%d): %s", j, rc, prev); return rc; }
        }
        npending = 0; groups = 0; side_used = true;
        return 0;
    };
    int mk = 0;
    auto do_marks = [&](int i) -> int {          // every mark at position i: both queues' events, behind everything issued so far
        while (mk < nmarks && marks[mk] <= i) {
            const int rc = flush(); if (rc) return rc;
            (void)hipEventRecord((hipEvent_t)ev_main[mk], ms);
            (void)hipEventRecord((hipEvent_t)ev_side[mk], ss);
            ++mk;
        }
        return 0;
    };
    for (int i = begin; i < end; ++i) {
        if (mk < nmarks) { const int rc = do_marks(i); if (rc) return rc; }
        const bool side = e[i].stream == 1;
        if (fork_every > 1) {
            if (side) {
                if (npending == 64) { const int rc = flush(); if (rc) return rc; }
                pending[npending++] = i; prev_side = true;
                continue;
            }
            if (prev_side) { ++groups; prev_side = false; }
            if (groups >= fork_every || e[i].stream == 2 || e[i].stream == 3) { const int rc = flush(); if (rc) return rc; }
        }
        if ((e[i].stream == 2 && side_used) || e[i].stream == 3) {   // a main-stream entry that consumes side-stream results:
            (void)hipEventRecord(g_events.ev[1], ss);                 // 2 = produced inside this range, 3 = enqueued on the side
            (void)hipStreamWaitEvent(ms, g_events.ev[1], 0);          // stream before the call (data-gradient weight packs)
            side_used = false;
        }
        if (side && main_dirty) {
            (void)hipEventRecord(g_events.ev[0], ms);
            (void)hipStreamWaitEvent(ss, g_events.ev[0], 0);
            main_dirty = false;
        }
        const bool handoff = !g_capturing && fork_every <= 1 && !side && i + 1 < end && e[i + 1].stream == 1;
        if (handoff) g_fork_event = g_events.ev[0];        // the entry may attach it to its last launch as the stop event
        const int rc = e[i].fn(e[i].args, side ? side_stream : main_stream);
        const bool taken = handoff && g_fork_event == nullptr;
        g_fork_event = nullptr;
        if (rc) {
            char prev[400];
            strncpy(prev, g_err, sizeof(prev) - 1); prev[sizeof(prev) - 1] = 0;
            salt_set_error("program entry %d failed (%d): %s", i, rc, prev);
            return rc;
        }
        if (side) side_used = true;
        else if (taken) { (void)hipStreamWaitEvent(ss, g_events.ev[0], 0); main_dirty = false; }
        else main_dirty = true;
    }
    { const int rc = flush(); if (rc) return rc; }
    if (mk < nmarks) { const int rc = do_marks(end); if (rc) return rc; }
    if (side_used && join_at_end) {
        (void)hipEventRecord(g_events.ev[1], ss);
        (void)hipStreamWaitEvent(ms, g_events.ev[1], 0);
    }
    return SALT_OK;
}

extern "C" int salt_program_run(const salt_program_entry* e, int n, void* stream) {
    return salt_program_run_range(e, 0, n, stream);
}

extern "C" int salt_graph_capture(const salt_program_entry* e, int n, void* stream, void** out) {
    if (!out || !stream) SALT_FAIL(SALT_E_BADARG, "graph capture needs a non-default stream");
    hipStream_t st = (hipStream_t)stream;
    hipError_t err = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
    if (err != hipSuccess) SALT_FAIL((int)err, "hipStreamBeginCapture: %s", hipGetErrorString(err));
    const int rc = salt_program_run(e, n, stream);
    hipGraph_t graph = nullptr;
    err = hipStreamEndCapture(st, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (err != hipSuccess) SALT_FAIL((int)err, "hipStreamEndCapture: %s", hipGetErrorString(err));
    hipGraphExec_t exec = nullptr;
    err = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (err != hipSuccess) SALT_FAIL((int)err, "hipGraphInstantiate: %s", hipGetErrorString(err));
    *out = (void*)exec;
    return SALT_OK;
}

// Capture of a whole step (several programs, two streams): bracket any sequence of salt_program_run* calls.  The side stream joins
// the capture through the executor's own event forks and must have re-joined `stream` (join_at_end) before salt_graph_end.
extern "C" int salt_graph_begin(void* stream) {
    if (!stream) SALT_FAIL(SALT_E_BADARG, "graph capture needs a non-default stream");
    hipError_t err = hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal);
    if (err != hipSuccess) SALT_FAIL((int)err, "hipStreamBeginCapture: %s", hipGetErrorString(err));
    g_capturing = true;
    return SALT_OK;
}

extern "C" int salt_graph_end(void* stream, void** out) {
    g_capturing = false;
    if (!stream || !out) SALT_FAIL(SALT_E_BADARG, "graph_end: bad args");
    hipGraph_t graph = nullptr;
    hipError_t err = hipStreamEndCapture((hipStream_t)stream, &graph);
    if (err != hipSuccess) { if (graph) (void)hipGraphDestroy(graph); SALT_FAIL((int)err, "hipStreamEndCapture: %s", hipGetErrorString(err)); }
    hipGraphExec_t exec = nullptr;
    err = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (err != hipSuccess) SALT_FAIL((int)err, "hipGraphInstantiate: %s", hipGetErrorString(err));
    *out = (void*)exec;
    return SALT_OK;
}

extern "C" int salt_graph_launch(void* exec, void* stream) {
    hipError_t err = hipGraphLaunch((hipGraphExec_t)exec, (hipStream_t)stream);
    if (err != hipSuccess) SALT_FAIL((int)err, "hipGraphLaunch: %s", hipGetErrorString(err));
    return SALT_OK;
}

extern "C" int salt_graph_destroy(void* exec) {
    if (exec) (void)hipGraphExecDestroy((hipGraphExec_t)exec);
    return SALT_OK;
}

__global__ void zero_kernel(uint32_t* p, int64_t n4) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) p[i] = 0u;
}

extern "C" int salt_zero(const salt_zero_args* a, void* stream) {
    if (!a || !a->p || a->bytes < 0 || (a->bytes & 3)) SALT_FAIL(SALT_E_BADARG, "zero: bad args");
    if (a->bytes == 0) return SALT_OK;
    const int64_t n4 = a->bytes / 4;
    const int blocks = (int)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
    return salt_launch(zero_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (uint32_t*)a->p, n4);
}

// sizeof() of every struct of saltnet.h in declaration order: the Python host compares them with its
// ctypes mirror at import so that a layout mismatch can never go unnoticed.
extern "C" int salt_abi_struct_sizes(int* out, int n) {
    static const int sizes[] = {
    (int)sizeof(salt_view),
    (int)sizeof(salt_conv_args),
    (int)sizeof(salt_conv_wgrad_args),
    (int)sizeof(salt_wgrad_reduce_args),
    (int)sizeof(salt_pack_conv_weight_args),
    (int)sizeof(salt_pack_batched_args),
    (int)sizeof(salt_conv_first_args),
    (int)sizeof(salt_conv_first_wgrad_args),
    (int)sizeof(salt_s2d_args),
    (int)sizeof(salt_pack_stem_weight_args),
    (int)sizeof(salt_stem_grad_unfold_args),
    (int)sizeof(salt_head1x1_args),
    (int)sizeof(salt_head1x1_bwd_args),
    (int)sizeof(salt_bn_finalize_args),
    (int)sizeof(salt_bn_fold_args),
    (int)sizeof(salt_affine_act_args),
    (int)sizeof(salt_bn_bwd_args),
    (int)sizeof(salt_head_bn_args),
    (int)sizeof(salt_head_bn_bwd_args),
    (int)sizeof(salt_relu_bwd_args),
    (int)sizeof(salt_maxpool2_args),
    (int)sizeof(salt_maxpool2_bwd_args),
    (int)sizeof(salt_avgpool2_args),
    (int)sizeof(salt_bilinear_args),
    (int)sizeof(salt_hyper_stencil_args),
    (int)sizeof(salt_pad_fold_args),
    (int)sizeof(salt_pad_fold_strip_args),
    (int)sizeof(salt_add_args),
    (int)sizeof(salt_layout_args),
    (int)sizeof(salt_scse_args),
    (int)sizeof(salt_scse_bwd_args),
    (int)sizeof(salt_depth_gate_args),
    (int)sizeof(salt_channel_gate_args),
    (int)sizeof(salt_lovasz_args),
    (int)sizeof(salt_bce_dice_args),
    (int)sizeof(salt_softmax_args),
    (int)sizeof(salt_softmax_bwd_args),
    (int)sizeof(salt_lovasz_softmax_args),
    (int)sizeof(salt_dice_ce_args),
    (int)sizeof(salt_adam_args),
    (int)sizeof(salt_adam_pack_args),
    (int)sizeof(salt_adam_tick_args),
    (int)sizeof(salt_zero_args),
    (int)sizeof(salt_tta_mean_args),
    (int)sizeof(salt_flip_args),
    (int)sizeof(salt_preprocess_args),
    (int)sizeof(salt_augment_config),
    (int)sizeof(salt_augment_preprocess_args),
    (int)sizeof(salt_crop_threshold_args),
    (int)sizeof(salt_iou_sweep_args),
    (int)sizeof(salt_stack_resize_args),
    (int)sizeof(salt_mask_resize_args),
    (int)sizeof(salt_resize_prob_args),
    (int)sizeof(salt_resize_threshold_args),
    (int)sizeof(salt_resize_iou_sweep_args),
    (int)sizeof(salt_ensemble_args),
    (int)sizeof(salt_rle_encode_args),
    (int)sizeof(salt_program_entry),
    (int)sizeof(salt_pool_head_args),
    (int)sizeof(salt_pool_head_bwd_args),
    (int)sizeof(salt_stack_conv_args),
    (int)sizeof(salt_stack_grad_unfold_args),
    (int)sizeof(salt_se_res_args),
    (int)sizeof(salt_se_res_bwd_args),
    (int)sizeof(salt_gconv_args),
    (int)sizeof(salt_gconv_dgrad_args),
    (int)sizeof(salt_gconv_wgrad_args),
    (int)sizeof(salt_dense_conv_args),
    (int)sizeof(salt_dense_conv_dgrad_args),
    (int)sizeof(salt_dense_conv_wgrad_args),
    (int)sizeof(salt_dense_moments_args),
    (int)sizeof(salt_dense_bn_prep_args),
    (int)sizeof(salt_gcn_pair_args),
    (int)sizeof(salt_gcn_pair_dgrad_args),
    (int)sizeof(salt_psp_pool_args),
    (int)sizeof(salt_psp_pool_bwd_args),
    (int)sizeof(salt_psp_merge_args),
    (int)sizeof(salt_psp_merge_bwd_args),
    (int)sizeof(salt_bn_prelu_args),
    (int)sizeof(salt_bn_prelu_bwd_args)};
    const int m = (int)(sizeof(sizes) / sizeof(sizes[0]));
    for (int i = 0; i < n && i < m; ++i) out[i] = sizes[i];
    return m;
}
