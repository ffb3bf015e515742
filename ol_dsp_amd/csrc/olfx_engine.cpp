// ol_dsp_amd/csrc/olfx_engine.cpp -- host side of libolfx.so: the C-ABI of include/olfx.h.
//
// Owns all device state of an engine (SoA rings, recursive scalars, derived coefficients), delivers
// the control packets that the host shadow (olfx_host.h: parameters, validation, coefficient
// derivation, packet format) fills at block boundaries, and launches the gfx950 kernels on a HIP
// stream.  There is no CPU compute path: if no GPU is present olfx_create fails with
// OLFX_E_NODEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/olfx.h"
#include "olfx_host.h"
#include "olfx_internal.h"

using namespace olfx;
using host::in_channels;
using host::out_channels;

namespace {

std::mutex g_err_mu;
std::string g_err;

void set_global_error(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> lk(g_err_mu);
    g_err = buf;
}

}  // namespace

// for the per-sample pool (olfx_sample_pool.cpp): its failures are reported through
// olfx_last_error(NULL) like engine-less errors here
void olfx::internal_set_error(const char *msg) { set_global_error("%s", msg); }

// ---------------------------------------------------------------------------------------------
// Engine
// ---------------------------------------------------------------------------------------------
struct olfx_engine {
    int kind = 0;
    int device = 0;
    uint32_t n = 0;
    uint32_t block = 0;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;    // copies of large control packets
    uint64_t frames = 0;
    std::string err;

    // user parameters, what of them the device has yet to see, and the queued note events
    host::Shadow hs;
    int cus = 0;                          // compute units (the chain's persistent grid)

    // control packets: a block's changed coefficients and folded note events, in pinned host
    // slots the block's kernels read (submit_control).  A slot is rewritten only after the
    // kernels that read it are done (consumed).
    // 16 slots in groups of 4: one `consumed` marker per group (each marker is a command-processor
    // packet between two blocks' kernels), recorded after the group's last packet or when the
    // caller switches streams; a slot's guard is its group's marker
    static constexpr int kSlots = 16, kGroup = 4, kBig = 2;
    static constexpr size_t kCopyBytes = 64 * 1024;   // packets from this size on are copied
    size_t copy_bytes = kCopyBytes;                  // OLFX_COPY_BYTES overrides (A/B diagnostic)
    struct Slot {
        uint32_t *h = nullptr, *hd = nullptr;   // pinned host half and its device address
        uint32_t *d = nullptr;                  // device half (large packets), allocated on first need
        size_t cap = 0, dcap = 0;               // words
        hipEvent_t copied = nullptr, consumed = nullptr;
        hipEvent_t guard = nullptr;             // the marker after this slot's last readers
        bool used = false;
    } slot[kSlots], big[kBig];                  // small packets (zero-copy) / large ones (copied)
    int slot_next = 0, big_next = 0;
    template <class F>
    void each_slot(F &&f) {
        for (Slot &x : slot) f(x);
        for (Slot &x : big) f(x);
    }
    int pending[kGroup] = {};                   // slots used since the last marker, all on pending_stream
    int n_pending = 0;
    hipStream_t pending_stream = nullptr;
    // the stream of the engine's latest launch (olfx_process / olfx_mix): what reset, sync and
    // destroy wait for (engine-scoped; the caller keeps that stream alive until then, olfx.h).  A
    // block on another stream is ordered after it through `switched` (recorded on the old stream at
    // the switch only: an event per block would cost a command-processor packet per block)
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    hipEvent_t switched = nullptr;
    // OLFX_TRACE_CONTROL=1 (read at create): host time of each control-path step, summed and
    // printed to stderr at destroy (tracing)
    bool trace = false;
    double tr[6] = {0, 0, 0, 0, 0, 0};
    uint64_t tr_calls = 0;

    // device memory: one allocation per engine, carved (carve)
    void *d_mem = nullptr;
    size_t d_bytes = 0;

    // fx rack
    float *fr_ring = nullptr;
    uint32_t *fr_state = nullptr, *fr_coef = nullptr;

    // dattorro (also the chain's reverb stage)
    uint32_t n_dt = 0;           // reverb-stage instances: n, or n rounded up to 64 for the chain and the plate rack
    float *dt_rings = nullptr;
    float *dt_state = nullptr;
    float *dt_coef = nullptr;
    // standalone reverb: the network (dattorro.hip dattorro_network) and so its pre-delay ring's
    // layout; re-decided at the next block after a pre-delay changed (hs.pre_changed)
    float *dt_pre_tmp = nullptr; // a copy of the pre-delay ring while its layout changes
    int dt_net = DT_NET_V4;      // the network of the last block; its pre-delay ring layout: rows unless v4

    // chorus / pitch-shift (also the chain's first two stages)
    uint32_t psize = 0, csize = 0;
    uint32_t pmax = 0;           // the pitch delay clamp: the pitch window's bound, whatever psize (ChorusArgs::pmax)
    float *ch_pring = nullptr, *ch_cring = nullptr;
    uint32_t *ch_state = nullptr, *ch_coef = nullptr;
    float *ps_pring = nullptr, *ps_cring = nullptr;      // chain stage 2
    uint32_t *ps_state = nullptr, *ps_coef = nullptr;

    // voice
    float *vc_state = nullptr, *vc_coef = nullptr;
    // sample voices: each voice's Sample ([SMC_N][n], in d_mem) and the bank (an allocation of its own:
    // configuration, kept by olfx_reset)
    uint32_t *sm_asg = nullptr;
    float *sm_bank = nullptr;
    uint64_t sm_bank_bytes = 0;
    // the drum kit: each kit's sum order ([n], DKC_ORDER); its voices' planes are vc_state, vc_coef and sm_asg
    // over the voice slots
    uint32_t *dk_order = nullptr;
    // the level meters: every signal's five floats ([MTS_N][channels * n]) and each instance's window and hold
    float *mt_state = nullptr, *mt_coef = nullptr;
    // voice buses (olfx_mix_config): [n_buses + 1] offsets, then the voice lists
    uint32_t *mix_dev = nullptr;
    uint32_t mix_quad = 0;                  // contiguous buses on multiples of 4 voices (voice_mix_v4)
    hipEvent_t mix_done = nullptr;          // recorded after every olfx_mix launch
    uint32_t n_buses = 0;

    // host-pointer I/O staging
    float *h_in = nullptr, *h_out = nullptr, *d_in = nullptr, *d_out = nullptr;
    size_t stage_floats_in = 0, stage_floats_out = 0;
    // device staging of frame tiles whose channel planes are too far apart for the kernels'
    // 32-bit buffer offsets (olfx_process on > 4 GiB planes), allocated on first need
    float *tile_in = nullptr, *tile_out = nullptr;
    size_t tile_floats = 0;

    int fail(int code, const char *fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        set_global_error("%s", buf);
        return code;
    }
    int hip_fail(hipError_t e, const char *what) {
        return fail(OLFX_E_HIP, "%s: %s", what, hipGetErrorString(e));
    }
    // the status of a host-shadow operation: its message becomes the engine's error
    int report(int rc) { return rc ? fail(rc, "%s", hs.msg) : OLFX_OK; }
};

#define HIPCHK(e, call)                                          \
    do {                                                         \
        hipError_t _r = (call);                                  \
        if (_r != hipSuccess) return (e)->hip_fail(_r, #call);   \
    } while (0)

namespace {

// The engine's device arrays: which a kind has, in allocation order, each on a 256-byte boundary.
// Without `base` only the size of the allocation is computed; with it the pointers are assigned.
size_t carve(olfx_engine *e, char *base) {
    size_t off = 0;
    auto take = [&](auto *&p, size_t bytes) {
        if (base) p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + off);
        off = (off + bytes + 255) / 256 * 256;
    };
    const int kind = e->kind;
    const size_t n = e->n, nd = e->n_dt;
    if (kind == OLFX_KIND_FXRACK || kind == OLFX_KIND_PLATERACK || is_synth_kind(kind) || kind == OLFX_KIND_DRUMKIT) {
        take(e->fr_ring, (size_t)kFrMaxDelay * 2 * n * 4);
        take(e->fr_state, (size_t)FRS_N * n * 4);
        take(e->fr_coef, (size_t)FRC_N * n * 4);
    }
    if (kind == OLFX_KIND_DATTORRO || kind == OLFX_KIND_CHAIN || kind == OLFX_KIND_PLATERACK) {
        take(e->dt_rings, (size_t)dt_total_floats() * nd * 4);
        take(e->dt_state, (size_t)DTS_N * nd * 4);
        take(e->dt_coef, (size_t)DTC_N * nd * 4);
    }
    if (kind == OLFX_KIND_CHORUS || kind == OLFX_KIND_PITCHSHIFT || kind == OLFX_KIND_CHAIN) {
        take(e->ch_pring, (size_t)2 * e->psize * n * 4);
        take(e->ch_cring, (size_t)2 * e->csize * n * 4);
        take(e->ch_state, (size_t)CHS_N * n * 4);
        take(e->ch_coef, (size_t)CHC_N * n * 4);
    }
    if (kind == OLFX_KIND_CHAIN) {
        take(e->ps_pring, (size_t)2 * e->psize * n * 4);
        take(e->ps_cring, 256);                          // the pitch-shift stage has no chorus ring
        take(e->ps_state, (size_t)CHS_N * n * 4);
        take(e->ps_coef, (size_t)CHC_N * n * 4);
    }
    if (is_voice_kind(kind)) {
        take(e->vc_state, (size_t)voice_state_slots(kind) * n * 4);
        take(e->vc_coef, (size_t)VCC_N * n * 4);
    }
    if (kind == OLFX_KIND_VOICE_SAMPLE) take(e->sm_asg, (size_t)SMC_N * n * 4);
    if (is_synth_kind(kind)) {
        // every voice slot's state (voices x n rounded up to 64); one set of coefficients per instrument
        take(e->vc_state, (size_t)voice_state_slots(kind) * e->hs.n_ev() * 4);
        take(e->vc_coef, (size_t)VCC_N * n * 4);
    }
    if (kind == OLFX_KIND_DRUMKIT) {
        // every voice slot's state, coefficients and Sample (voices x n rounded up to 64); the kits' sum orders
        const size_t slots = e->hs.n_ev();
        take(e->vc_state, (size_t)VCS_N * slots * 4);
        take(e->vc_coef, (size_t)VCC_N * slots * 4);
        take(e->sm_asg, (size_t)SMC_N * slots * 4);
        take(e->dk_order, (size_t)DKC_N * n * 4);
    }
    if (is_meter_kind(kind)) {
        take(e->mt_state, (size_t)MTS_N * in_channels(kind) * n * 4);
        take(e->mt_coef, (size_t)MTC_N * n * 4);
    }
    return off;
}

// ---------------------------------------------------------------------------------------------
// Control path (parameters and note events at the block boundary; JUCE-host pattern,
// modules/juce/host/host.cpp:646-653): O(changed), asynchronous, no host<->device round trip.
// ---------------------------------------------------------------------------------------------

// The destination arrays (field-major, CoefScatterArgs) of a coefficient record's segments: each part
// of the kind goes to the array its row names (host::Dst); returns the record's words.  voice_slots: the
// record of a kit kind's voice slot instead (KindDesc::vparts).
uint32_t coef_segments(const olfx_engine *e, CoefScatterArgs *a, bool voice_slots = false) {
    const host::KindDesc &kd = *e->hs.kd;
    // a kit's voice arrays are indexed by voice slot (p * npad + kit)
    const uint32_t nv = kd.voice_slots ? e->hs.n_ev() : e->n;
    const struct { void *p; uint32_t stride; } to[host::TO_COUNT] = {
        /* TO_DT */ {e->dt_coef, e->n_dt},       // padding plate instances keep their zeroed coefficients
        /* TO_CH */ {e->ch_coef, e->n},
        /* TO_PS */ {e->ps_coef, e->n},
        /* TO_VC */ {e->vc_coef, nv},
        /* TO_FR */ {e->fr_coef, e->n},
        /* TO_SM */ {e->sm_asg, nv},
        /* TO_ORD */ {e->dk_order, e->n},
        /* TO_MT */ {e->mt_coef, e->n},
    };
    const host::Segments sg = voice_slots ? host::voice_segments(e->kind) : host::coef_segments(e->kind);
    const host::Part *parts = voice_slots ? kd.vparts : kd.parts;
    a->nseg = sg.nseg;
    for (uint32_t k = 0; k < sg.nseg; ++k) {
        a->dst[k] = (uint32_t *)to[parts[k].dst].p;
        a->words[k] = sg.words[k];
        a->stride[k] = to[parts[k].dst].stride;
    }
    return voice_slots ? kd.vwords : kd.words;
}

// Record one marker after the pending slots' kernels (on their stream) and make it their guard.
hipError_t flush_markers(olfx_engine *e) {
    if (!e->n_pending) return hipSuccess;
    hipEvent_t m = e->slot[e->pending[e->n_pending - 1]].consumed;
    const hipError_t r = hipEventRecord(m, e->pending_stream);
    for (int k = 0; k < e->n_pending; ++k) e->slot[e->pending[k]].guard = r == hipSuccess ? m : nullptr;
    e->n_pending = 0;
    return r;
}

// A block's kernels that read slot `sl` are queued on `s`: a big slot gets its own marker, a small
// one joins the pending group.
hipError_t slot_queued(olfx_engine *e, olfx_engine::Slot *sl, hipStream_t s) {
    if (sl >= e->big && sl < e->big + olfx_engine::kBig) {
        const hipError_t r = hipEventRecord(sl->consumed, s);
        sl->guard = r == hipSuccess ? sl->consumed : nullptr;
        return r;
    }
    hipError_t r = hipSuccess;
    if (e->n_pending && e->pending_stream != s) r = flush_markers(e);
    e->pending[e->n_pending++] = (int)(sl - e->slot);
    e->pending_stream = s;
    if (e->n_pending == olfx_engine::kGroup) {
        const hipError_t r2 = flush_markers(e);
        if (r == hipSuccess) r = r2;
    }
    return r;
}

// A slot's pinned half (and, for copied packets, its device half) of at least `words` words.
int grow_slot(olfx_engine *e, olfx_engine::Slot &sl, size_t words, bool device_half) {
    if (sl.cap < words) {
        if (sl.h) (void)hipHostFree(sl.h);
        sl.h = nullptr; sl.hd = nullptr; sl.cap = 0;
        const size_t cap = std::max<size_t>(words, 4096);
        // zero-copy slots (read by the kernels over the host link, rewritten 16 blocks later) are
        // coherent: no GPU cache may hold a stale line of them whatever HIP_HOST_COHERENT says;
        // copied slots are only a copy source
        HIPCHK(e, hipHostMalloc((void **)&sl.h, cap * 4,
                                device_half ? hipHostMallocDefault : (hipHostMallocMapped | hipHostMallocCoherent)));
        void *dp = nullptr;
        HIPCHK(e, hipHostGetDevicePointer(&dp, sl.h, 0));
        sl.hd = (uint32_t *)dp;
        sl.cap = cap;
    }
    if (device_half && sl.dcap < sl.cap) {
        if (sl.d) (void)hipFree(sl.d);
        sl.d = nullptr; sl.dcap = 0;
        HIPCHK(e, hipMalloc((void **)&sl.d, sl.cap * 4));
        sl.dcap = sl.cap;
    }
    return OLFX_OK;
}

// The chorus kind's arrays and geometry for a launch whose first frame is the engine's next.
ChorusArgs chorus_args(const olfx_engine *e, uint32_t n_frames, uint64_t plane) {
    ChorusArgs a{};
    a.pitch_ring = e->ch_pring;
    a.chorus_ring = e->ch_cring;
    a.state = e->ch_state;
    a.coef = e->ch_coef;
    a.plane = plane;
    a.n = e->n;
    a.n_frames = n_frames;
    a.t0 = (uint32_t)(e->frames & 0xFFFFFFFFu);
    a.psize = e->psize;
    a.csize = e->csize;
    a.pmax = e->pmax;
    return a;
}

// This block's control packet -- the changed instances' coefficient records and the folded note
// events (host::PacketPlan) -- in a pinned host slot that the block's kernels read directly over
// the host link (zero-copy: no copy command, no second stream, no host wait on the device).  The
// coefficients are scattered on `s` ahead of the block's kernel; the voice kernel reads its events
// itself.  A slot is rewritten only after the kernels that read it are done (its `consumed` event,
// recorded by the caller after them: *used_slot).
// `span`: the frames of the launch the packet is for (timed events below it become its segments).
// `tp`: the packet's timed instrument section for the launch (the synths and the drum kit), if it has one.
int submit_control(olfx_engine *e, hipStream_t s, VoiceArgs *va, InstrumentTimed *tp, olfx_engine::Slot **used_slot,
                   uint32_t span) {
    *used_slot = nullptr;
    host::Shadow &hs = e->hs;
    const bool evs = host::takes_note_events(e->kind) && hs.has_events(span);
    const size_t m = hs.dirty_list.size(), m2 = hs.vdirty_list.size();    // (m2: a kit kind's voice slots)
    if (!m && !m2 && !evs) return OLFX_OK;
    using clk = std::chrono::steady_clock;
    auto t_prev = clk::now();
    auto lap = [&](int k) {
        if (!e->trace) return;
        const auto t = clk::now();
        e->tr[k] += std::chrono::duration<double, std::micro>(t - t_prev).count();
        t_prev = t;
    };
    e->tr_calls++;
    if (evs) hs.fold_segments(span);
    lap(0);
    CoefScatterArgs ca{};
    const uint32_t W = coef_segments(e, &ca);
    const host::PacketPlan pl = hs.plan(evs);

    // Delivery: a small packet (a block's CCs / notes) is read by the kernels straight from a pinned
    // slot -- no copy command: ~2 us of host time, a host-link round trip or two inside the kernel.
    // A large one (the first block's full upload, an all-voices note-off) goes to one of two big
    // slots and is copied into its device half on the engine's copy stream, which the caller's
    // stream waits for: ~20 us of host API time, but no 512-KB read over the host link on the
    // kernel's critical path.
    const bool copy = pl.words * 4 >= e->copy_bytes;
    olfx_engine::Slot &sl = copy ? e->big[e->big_next] : e->slot[e->slot_next];
    if (copy) e->big_next = (e->big_next + 1) % olfx_engine::kBig;
    else e->slot_next = (e->slot_next + 1) % olfx_engine::kSlots;
    // the slot is free once the kernels that read it are done (both halves)
    if (sl.used) {
        if (!sl.guard) HIPCHK(e, flush_markers(e));
        if (sl.guard) HIPCHK(e, hipEventSynchronize(sl.guard));
        else HIPCHK(e, hipDeviceSynchronize());     // its marker failed to record: wait for everything
    }
    lap(1);
    if (const int rc = grow_slot(e, sl, pl.words, copy)) return rc;
    uint32_t *const dev = copy ? sl.d : sl.hd;      // what the kernels read
    lap(2);
    hs.fill_records(pl, sl.h);
    if (hs.rf_materialise) {
        // a pitch or window change ends ring-free mode: the chorus ring's history from the x ring, under
        // the coefficients still on the device (ahead of the scatter below)
        hs.rf_materialise = false;
        const hipError_t r = launch_chorus_materialise(chorus_args(e, 0, 0), hs.rf.depth, s);
        if (r != hipSuccess) return e->hip_fail(r, "chorus ring materialise launch");
    }
    lap(3);
    if (evs) hs.write_events(sl.h + pl.o_ev);
    if (pl.n_tc) hs.write_timed_coefs(pl, sl.h);
    if (pl.n_iv + pl.n_if) hs.write_timed_inst(pl, sl.h);
    if (copy) {
        // the copy stream waits for nothing on the device: the host made sure above that the slot's
        // previous readers are done (a device-side wait there serialised the copy behind them)
        HIPCHK(e, hipMemcpyAsync(sl.d, sl.h, pl.words * 4, hipMemcpyHostToDevice, e->copy_stream));
        HIPCHK(e, hipEventRecord(sl.copied, e->copy_stream));
        HIPCHK(e, hipStreamWaitEvent(s, sl.copied, 0));
    } else {
        std::atomic_thread_fence(std::memory_order_seq_cst);     // the packet's stores before the launch
    }
    sl.used = true;
    sl.guard = nullptr;
    *used_slot = &sl;
    lap(4);
    if (m) {
        ca.inst = pl.dense ? nullptr : dev + pl.o_inst;
        ca.val = dev + pl.o_val;
        ca.m = (uint32_t)m;
        ca.W = W;
        const hipError_t r = launch_coef_scatter(ca, s);
        if (r != hipSuccess) return e->hip_fail(r, "coefficient scatter launch");
    }
    if (m2) {
        CoefScatterArgs cv{};
        cv.W = coef_segments(e, &cv, true);
        cv.inst = dev + pl.o_inst2;
        cv.val = dev + pl.o_val2;
        cv.m = (uint32_t)m2;
        const hipError_t r = launch_coef_scatter(cv, s);
        if (r != hipSuccess) return e->hip_fail(r, "voice-slot coefficient scatter launch");
    }
    if (evs) {
        va->ev = reinterpret_cast<const uint2 *>(dev + pl.o_ev);
        va->ev_more = va->ev + pl.n_seg * (size_t)((hs.n_ev() + 63u) / 64u) * kVevCap;
        if (pl.n_seg > 1) {               // timed events: the segmented kernel
            va->n_seg = (uint32_t)pl.n_seg;
            va->n_chunks = hs.n_chunks(span, kVoiceChunk);
            va->seg = dev + pl.o_seg;
            if (pl.n_tc) {                // timed parameters: the segments' coefficient records
                va->tc_base = dev + pl.o_tcb;
                va->tc = dev + pl.o_tc;
                va->tc_n = (uint32_t)pl.n_tc;
            }
            if (pl.n_iv + pl.n_if) {      // timed instrument parameters: the segments' voice and rack records
                tp->vtab = reinterpret_cast<const uint4 *>(dev + pl.o_ivt);
                tp->ftab = reinterpret_cast<const uint4 *>(dev + pl.o_ift);
                tp->vrec = reinterpret_cast<const float *>(dev + pl.o_iv);
                tp->frec = dev + pl.o_if;
                tp->n_v = (uint32_t)pl.n_iv;
                tp->n_f = (uint32_t)pl.n_if;
                tp->gv = (uint32_t)pl.gv;
            }
        }
    }
    lap(5);
    return OLFX_OK;
}

// A call on `s` after the engine's previous launch, whichever stream that was on.
int order_after_last(olfx_engine *e, hipStream_t s) {
    if (e->have_last && s != e->last_stream) {
        HIPCHK(e, hipEventRecord(e->switched, e->last_stream));
        HIPCHK(e, hipStreamWaitEvent(s, e->switched, 0));
    }
    return OLFX_OK;
}
// The engine's latest launch is on `s`.
void launched_on(olfx_engine *e, hipStream_t s) {
    e->last_stream = s;
    e->have_last = true;
}

// Wait for this engine's queued work only -- not the device: its latest launch stream (the caller
// orders its own streams, so that covers every earlier block), its own stream, and every control
// slot's marker.  A slot whose marker failed to record falls back to a device-wide wait.
int wait_engine(olfx_engine *e) {
    HIPCHK(e, flush_markers(e));
    bool unmarked = false;
    e->each_slot([&](olfx_engine::Slot &sl) {
        if (!sl.used) return;
        if (sl.guard) {
            if (hipEventSynchronize(sl.guard) != hipSuccess) unmarked = true;
        } else {
            unmarked = true;
        }
        if (sl.d && sl.copied && hipEventSynchronize(sl.copied) != hipSuccess) unmarked = true;
    });
    if (e->mix_done) HIPCHK(e, hipEventSynchronize(e->mix_done));
    if (e->have_last) HIPCHK(e, hipStreamSynchronize(e->last_stream));
    if (e->stream) HIPCHK(e, hipStreamSynchronize(e->stream));
    if (e->copy_stream) HIPCHK(e, hipStreamSynchronize(e->copy_stream));
    if (unmarked) HIPCHK(e, hipDeviceSynchronize());
    return OLFX_OK;
}

// Every instance back to the freshly created state.  The caller has made sure that none of the
// engine's work is still queued (olfx_create: none was; olfx_reset: wait_engine).
int init_state(olfx_engine *e) {
    e->n_pending = 0;
    e->each_slot([](olfx_engine::Slot &sl) { sl.used = false; sl.guard = nullptr; });
    HIPCHK(e, hipMemsetAsync(e->d_mem, 0, e->d_bytes, e->stream));
    // voices: daisysp Oscillator::Init phase 0; Svf::Init states 0; Adsr idle; freq_ = 0
    // (SynthVoice.h:276); Port z1 = 0 -- all zeros
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->hs.reset();                 // defaults; every coefficient is derived at the first block
    e->dt_net = DT_NET_V4;         // the zeroed ring is valid in either layout: decided at the next block
    e->frames = 0;
    return OLFX_OK;
}

// A (pinned, device) staging pair of at least `floats` floats.
int grow_staging(olfx_engine *e, float *&h, float *&d, size_t &have, size_t floats) {
    if (floats <= have) return OLFX_OK;
    if (h) (void)hipHostFree(h);
    if (d) (void)hipFree(d);
    h = nullptr; d = nullptr;
    HIPCHK(e, hipHostMalloc((void **)&h, floats * 4, hipHostMallocDefault));
    HIPCHK(e, hipMalloc((void **)&d, floats * 4));
    have = floats;
    return OLFX_OK;
}
int ensure_staging(olfx_engine *e, size_t fin, size_t fout) {
    if (const int rc = grow_staging(e, e->h_in, e->d_in, e->stage_floats_in, fin)) return rc;
    return grow_staging(e, e->h_out, e->d_out, e->stage_floats_out, fout);
}

// One launch over frames [e->frames, e->frames + n_frames) of every instance: in / out hold those
// frames with channel planes `plane` floats apart.  `ev` carries the block's note events (voices).
int launch(olfx_engine *e, const float *din, float *dout, uint32_t n_frames, uint64_t plane, hipStream_t s,
           const VoiceArgs &ev, const InstrumentTimed &tp) {
    hipError_t r = hipSuccess;
    const uint32_t t0 = (uint32_t)(e->frames & 0xFFFFFFFFu);
    auto dt_args = [&](const float *in, float *out) {
        DattorroArgs a{};
        size_t off = 0;
        for (int l = 0; l < DT_NLINES; ++l) {
            a.ring[l] = e->dt_rings + off;
            off += (size_t)kDtSize[l] * e->n_dt;
        }
        a.state = e->dt_state;
        a.coef = e->dt_coef;
        a.in = in;
        a.out = out;
        a.plane = plane;
        a.n = e->n_dt;
        a.n_frames = n_frames;
        a.t0 = t0 & 0xFFFFu;
        a.in_ch = 2;
        a.cus = (uint32_t)e->cus;
        return a;
    };
    auto ch_args = [&](float *pr, float *cr, uint32_t *st, const uint32_t *cf, const float *in,
                       float *out, uint32_t mode) {
        ChorusArgs a{};
        a.pitch_ring = pr;
        a.chorus_ring = cr;
        a.state = st;
        a.coef = cf;
        a.in = in;
        a.out = out;
        a.plane = plane;
        a.n = e->n;
        a.n_frames = n_frames;
        a.t0 = t0;
        a.psize = e->psize;
        a.csize = e->csize;
        a.pmax = e->pmax;
        a.mode = mode;
        return a;
    };
    // what the fused instrument kinds share (synth, Svf synth, drum kit)
    auto instrument_args = [&](InstrumentArgs &a) {
        a.ring = e->fr_ring;
        a.fr_state = e->fr_state;
        a.fr_coef = e->fr_coef;
        a.vc_state = e->vc_state;
        a.vc_coef = e->vc_coef;
        a.out = dout;
        a.plane = plane;
        a.n = e->n;
        a.n_frames = n_frames;
        a.t0 = (uint32_t)(e->frames % kFrMaxDelay);
        a.voices = e->hs.voices;
        a.npad = e->hs.npad;
        a.ev = ev.ev;
        a.ev_more = ev.ev_more;
        a.n_seg = ev.n_seg;               // timed notes: the *_seg kernel
        a.seg = ev.seg;
    };
    switch (e->kind) {
    case OLFX_KIND_DATTORRO: {
        if (e->hs.pre_changed) {
            // one pre-delay for all instances or several: the network (dattorro.hip dattorro_network)
            // and so the pre-delay ring's layout; its content is converted when that changes
            e->hs.pre_changed = false;
            const int net = dattorro_network(e->n_dt, (uint32_t)e->cus, e->hs.uniform_predelay());
            const bool rows = net != DT_NET_V4;
            if (rows != (e->dt_net != DT_NET_V4) && e->frames > 0) {   // a fresh (zeroed) ring needs no conversion
                if (!e->dt_pre_tmp) HIPCHK(e, hipMalloc((void **)&e->dt_pre_tmp, (size_t)kDtSize[DT_PRE] * e->n_dt * 4));
                r = launch_dattorro_pre_layout(dt_args(nullptr, nullptr), e->dt_pre_tmp, rows, s);
                if (r != hipSuccess) return e->hip_fail(r, "pre-delay ring layout");
            }
            e->dt_net = net;
        }
        r = launch_dattorro(dt_args(din, dout), e->dt_net, s);
        break;
    }
    case OLFX_KIND_CHORUS: {
        // ring-free unless a pitch or window change is younger than the chorus history (host::RingFree)
        const ChorusArgs a = ch_args(e->ch_pring, e->ch_cring, e->ch_state, e->ch_coef, din, dout, 0);
        r = e->hs.rf.active() ? launch_chorus_ringfree(a, s) : launch_chorus(a, s);
        e->hs.rf.advance(n_frames);
        break;
    }
    case OLFX_KIND_PITCHSHIFT:
        r = launch_chorus(ch_args(e->ch_pring, e->ch_cring, e->ch_state, e->ch_coef, din, dout, 1), s);
        break;
    case OLFX_KIND_VOICE:
    case OLFX_KIND_VOICE_MOOG:
    case OLFX_KIND_VOICE_SAMPLE: {
        VoiceArgs a{};
        a.state = e->vc_state;
        a.coef = e->vc_coef;
        a.out = dout;
        a.n = e->n;
        a.n_frames = n_frames;
        a.moog = e->kind == OLFX_KIND_VOICE_MOOG;
        a.ev_more = ev.ev_more;
        a.ev = ev.ev;
        a.smp = e->sm_asg;
        a.bank = e->sm_bank;
        a.bank_bytes = (uint32_t)e->sm_bank_bytes;
        a.n_seg = ev.n_seg;
        a.n_chunks = ev.n_chunks;
        a.seg = ev.seg;
        a.tc_base = ev.tc_base;
        a.tc = ev.tc;
        a.tc_n = ev.tc_n;
        r = e->kind == OLFX_KIND_VOICE_SAMPLE ? launch_sampler(a, s) : launch_voice(a, s);
        break;
    }
    case OLFX_KIND_FXRACK: {
        FxRackArgs a{};
        a.ring = e->fr_ring;
        a.state = e->fr_state;
        a.coef = e->fr_coef;
        a.in = din;
        a.out = dout;
        a.plane = plane;
        a.n = e->n;
        a.n_frames = n_frames;
        a.t0 = (uint32_t)(e->frames % kFrMaxDelay);
        a.components = e->hs.n_components > 0;
        r = launch_fxrack(a, s);
        break;
    }
    case OLFX_KIND_PLATERACK: {
        // one fused launch: the delay waves feed the plate wave and the filter wave through LDS.  Two
        // clocks from the one frame count: the rack ring's position and the plate's 16-bit stream time
        PlateRackArgs a{};
        a.ring = e->fr_ring;
        a.state = e->fr_state;
        a.coef = e->fr_coef;
        a.d = dt_args(nullptr, nullptr);
        a.in = din;
        a.out = dout;
        a.plane = plane;
        a.n = e->n;
        a.n_frames = n_frames;
        a.t0 = (uint32_t)(e->frames % kFrMaxDelay);
        a.cus = (uint32_t)e->cus;
        r = launch_platerack(a, s);
        break;
    }
    case OLFX_KIND_SYNTH:
    case OLFX_KIND_SYNTH_SVF: {
        // one fused launch: the voice waves feed the delay waves and the filter wave through LDS
        SynthSegArgs a{};
        instrument_args(a);
        a.svf = e->kind == OLFX_KIND_SYNTH_SVF;
        a.tp = tp;
        r = launch_synth(a, s);
        break;
    }
    case OLFX_KIND_DRUMKIT: {
        // one fused launch: the sample-voice waves feed the delay waves and the filter wave through LDS
        DrumkitSegArgs a{};
        instrument_args(a);
        a.tp = tp;
        a.smp = e->sm_asg;
        a.order = e->dk_order;
        a.bank = e->sm_bank;
        a.bank_bytes = (uint32_t)e->sm_bank_bytes;
        r = launch_drumkit(a, s);
        break;
    }
    case OLFX_KIND_METER:
    case OLFX_KIND_METER_MONO: {
        // dout null: summary mode
        MeterArgs a{};
        a.in = din;
        a.out = dout;
        a.state = e->mt_state;
        a.coef = e->mt_coef;
        a.plane = plane;
        a.n = e->n;
        a.n_frames = n_frames;
        a.planes = in_channels(e->kind);
        r = launch_meter(a, s);
        break;
    }
    case OLFX_KIND_CHAIN: {
        // one fused launch: chorus and pitch-shift waves feed the reverb wave through LDS
        ChainArgs a{};
        a.c1 = ch_args(e->ch_pring, e->ch_cring, e->ch_state, e->ch_coef, nullptr, nullptr, 0);
        a.c2 = ch_args(e->ps_pring, e->ps_cring, e->ps_state, e->ps_coef, nullptr, nullptr, 1);
        a.d = dt_args(nullptr, nullptr);
        a.in = din;
        a.out = dout;
        a.plane = plane;
        a.n = e->n;
        a.n_frames = n_frames;
        a.cus = (uint32_t)e->cus;
        r = launch_chain(a, s);
        break;
    }
    default: return e->fail(OLFX_E_KIND, "unknown kind");
    }
    if (r != hipSuccess) return e->hip_fail(r, "kernel launch");
    return OLFX_OK;
}

// All n_frames of a call, as frame tiles where a launch's planes would leave the kernel's 32-bit
// offset range (KindDesc::planes_32bit): a tile is frames [f0, f0 + F) at in + f0 n with the caller's
// plane distance, so the launch spans plane + F n floats (< 4 GiB); when the caller's planes alone
// are >= 4 GiB apart, tiles are staged through a compact device buffer.  Frames run in order and
// the state carries between launches, so tiles compute exactly what one launch would.  The note
// events apply before the first tile (the block's start).
// `call_frames`: the frames of the whole olfx_process call, of which these n_frames are a run (timed events at
// more times than a launch takes: in / out point at the run's first frame, and the channel planes keep the
// call's distance).
int run_frames(olfx_engine *e, const float *in, float *out, uint32_t n_frames, uint32_t call_frames, hipStream_t s,
               const VoiceArgs &ev, const InstrumentTimed &tp) {
    const uint64_t n = e->n, plane = (uint64_t)call_frames * n;
    const uint64_t lim = (1ull << 30) - 1;                     // floats addressable in 32-bit bytes
    const VoiceArgs none{};
    const InstrumentTimed no_tp{};
    if (!e->hs.kd->planes_32bit || plane + plane <= lim) {
        const int rc = launch(e, in, out, n_frames, plane, s, ev, tp);
        if (rc) return rc;
        e->frames += n_frames;
        return OLFX_OK;
    }
    if (plane + 4 * n <= lim) {
        const uint32_t F = (uint32_t)std::min<uint64_t>(n_frames, ((lim - plane) / n) & ~3ull);
        for (uint32_t f0 = 0; f0 < n_frames; f0 += F) {
            const uint32_t Ft = std::min(F, n_frames - f0);
            const int rc = launch(e, in ? in + (size_t)f0 * n : nullptr, out + (size_t)f0 * n, Ft, plane, s,
                                  f0 ? none : ev, f0 ? no_tp : tp);
            if (rc) return rc;
            e->frames += Ft;
        }
        return OLFX_OK;
    }
    // staged: tiles of up to 256 MiB per direction, compact [ch][F][n]
    const uint32_t ich = in_channels(e->kind), och = out_channels(e->kind);
    const uint32_t F = (uint32_t)std::max<uint64_t>(4, std::min<uint64_t>(n_frames, ((1ull << 26) / (2 * n)) & ~3ull));
    if (e->tile_floats < (size_t)2 * F * n) {
        if (e->tile_in) (void)hipFree(e->tile_in);
        if (e->tile_out) (void)hipFree(e->tile_out);
        e->tile_in = e->tile_out = nullptr;
        e->tile_floats = 0;
        HIPCHK(e, hipMalloc((void **)&e->tile_in, (size_t)2 * F * n * 4));
        HIPCHK(e, hipMalloc((void **)&e->tile_out, (size_t)2 * F * n * 4));
        e->tile_floats = (size_t)2 * F * n;
    }
    for (uint32_t f0 = 0; f0 < n_frames; f0 += F) {
        const uint32_t Ft = std::min(F, n_frames - f0);
        const size_t bytes = (size_t)Ft * n * 4;
        for (uint32_t c = 0; c < ich; ++c)
            HIPCHK(e, hipMemcpyAsync(e->tile_in + (size_t)c * Ft * n, in + c * plane + (size_t)f0 * n, bytes,
                                     hipMemcpyDeviceToDevice, s));
        const int rc = launch(e, e->tile_in, e->tile_out, Ft, (uint64_t)Ft * n, s, f0 ? none : ev, f0 ? no_tp : tp);
        if (rc) return rc;
        for (uint32_t c = 0; c < och; ++c)
            HIPCHK(e, hipMemcpyAsync(out + c * plane + (size_t)f0 * n, e->tile_out + (size_t)c * Ft * n, bytes,
                                     hipMemcpyDeviceToDevice, s));
        e->frames += Ft;
    }
    return OLFX_OK;
}

}  // namespace

// =============================================================================================
// C-ABI
// =============================================================================================
extern "C" {

int olfx_abi_version(void) { return OLFX_ABI_VERSION; }

int olfx_kind_info_get(int kind, float sample_rate, olfx_kind_info *info) {
    if (!info) return OLFX_E_ARG;
    const uint32_t np = host::n_params_of(kind);
    if (!np) return OLFX_E_KIND;
    info->kind = kind;
    info->n_params = np;
    info->in_channels = in_channels(kind);
    info->out_channels = out_channels(kind);
    info->state_bytes_per_instance = host::state_bytes(kind, 1, sample_rate);
    return OLFX_OK;
}

static int create_engine(int kind, int device, uint32_t n_inst, uint32_t voices, float sample_rate, uint32_t block,
                         olfx_engine **out);

int olfx_create(int kind, int device, uint32_t n_inst, float sample_rate, uint32_t block,
                olfx_engine **out) {
    return create_engine(kind, device, n_inst, host::kSynthDefaultVoices, sample_rate, block, out);
}

int olfx_create_synth(int device, uint32_t n_inst, uint32_t voices, float sample_rate, uint32_t block,
                      olfx_engine **out) {
    if (!out) return OLFX_E_ARG;
    *out = nullptr;
    if (voices < 1 || voices > host::kSynthMaxVoices) {
        set_global_error("olfx_create_synth: %u voices per instrument (1..%u)", voices, host::kSynthMaxVoices);
        return OLFX_E_ARG;
    }
    return create_engine(OLFX_KIND_SYNTH, device, n_inst, voices, sample_rate, block, out);
}

int olfx_create_synth_kind(int kind, int device, uint32_t n_inst, uint32_t voices, float sample_rate, uint32_t block,
                           olfx_engine **out) {
    if (!out) return OLFX_E_ARG;
    *out = nullptr;
    if (!is_synth_kind(kind)) {
        set_global_error("olfx_create_synth_kind: kind %d is not a synth", kind);
        return OLFX_E_KIND;
    }
    if (voices < 1 || voices > host::kSynthMaxVoices) {
        set_global_error("olfx_create_synth_kind: %u voices per instrument (1..%u)", voices, host::kSynthMaxVoices);
        return OLFX_E_ARG;
    }
    return create_engine(kind, device, n_inst, voices, sample_rate, block, out);
}

int olfx_create_drumkit(int device, uint32_t n_kits, uint32_t voices, float sample_rate, uint32_t block,
                        olfx_engine **out) {
    if (!out) return OLFX_E_ARG;
    *out = nullptr;
    if (voices < 1 || voices > kDkMaxVoices) {
        set_global_error("olfx_create_drumkit: %u voices per kit (1..%u)", voices, kDkMaxVoices);
        return OLFX_E_ARG;
    }
    return create_engine(OLFX_KIND_DRUMKIT, device, n_kits, voices, sample_rate, block, out);
}

static int create_engine(int kind, int device, uint32_t n_inst, uint32_t voices, float sample_rate, uint32_t block,
                         olfx_engine **out) {
    if (!out) return OLFX_E_ARG;
    *out = nullptr;
    if (!host::n_params_of(kind)) {
        set_global_error("olfx_create: unknown kind %d", kind);
        return OLFX_E_KIND;
    }
    // (the synths' and the drum kit's voice slots, voices x n rounded up to 64, are indexed in 32 bits)
    const bool too_many = host::kind_desc(kind).instances == host::KindDesc::INSTRUMENTS && ((uint64_t)n_inst + 63u) / 64u * 64u * voices > 0x7FFFFFFFull;
    if (n_inst == 0 || too_many || !(sample_rate > 1000.f && sample_rate <= 384000.f) || block == 0 || (block & 3u)) {
        set_global_error("olfx_create: bad argument (n_inst=%u sr=%g block=%u)", n_inst, sample_rate, block);
        return OLFX_E_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_global_error("olfx_create: no HIP device visible (this library has no CPU path)");
        return OLFX_E_NODEVICE;
    }
    if (device < 0 || device >= ndev) {
        set_global_error("olfx_create: device %d out of range (%d devices)", device, ndev);
        return OLFX_E_NODEVICE;
    }
    olfx_engine *e = new (std::nothrow) olfx_engine();
    if (!e) return OLFX_E_NOMEM;
    e->kind = kind;
    e->device = device;
    e->n = n_inst;
    e->block = block;
    e->hs.init(kind, n_inst, sample_rate, voices);
    e->trace = std::getenv("OLFX_TRACE_CONTROL") && std::getenv("OLFX_TRACE_CONTROL")[0] == '1';
    if (const char *cb = std::getenv("OLFX_COPY_BYTES"))
        e->copy_bytes = std::min<size_t>((size_t)std::strtoull(cb, nullptr, 10), olfx_engine::kCopyBytes);
    host::chorus_sizes(sample_rate, &e->psize, &e->csize);
    e->pmax = e->psize - 2u;
    // the chorus kind's x ring also holds the chorus history (chorus_stage_rf.h)
    if (kind == OLFX_KIND_CHORUS) e->psize = host::chorus_x_size(sample_rate);
    e->n_dt = e->hs.kd->pad_plate ? (n_inst + 63u) & ~63u : n_inst;

    hipError_t r = hipSetDevice(device);
    if (r == hipSuccess) r = hipDeviceGetAttribute(&e->cus, hipDeviceAttributeMultiprocessorCount, device);
    if (r == hipSuccess) r = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (r == hipSuccess) r = hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking);
    if (r == hipSuccess) r = hipEventCreateWithFlags(&e->switched, hipEventDisableTiming);
    e->each_slot([&](olfx_engine::Slot &x) {
        if (r == hipSuccess) r = hipEventCreateWithFlags(&x.copied, hipEventDisableTiming);
        if (r == hipSuccess) r = hipEventCreateWithFlags(&x.consumed, hipEventDisableTiming);
    });
    if (r != hipSuccess) {
        int rc = e->hip_fail(r, "olfx_create: stream / events");
        olfx_destroy(e);
        return rc;
    }

    e->d_bytes = carve(e, nullptr);
    r = hipMalloc(&e->d_mem, e->d_bytes);
    if (r != hipSuccess) {
        int rc = e->fail(OLFX_E_NOMEM, "olfx_create: hipMalloc(%zu bytes): %s", e->d_bytes, hipGetErrorString(r));
        e->d_mem = nullptr;
        olfx_destroy(e);
        return rc;
    }
    carve(e, (char *)e->d_mem);
    int rc = init_state(e);
    // slots allocated now, so that no block -- an all-voices note-off in the middle of a stream,
    // say -- pays a pinned / device allocation: the small ones at the copy threshold, the big ones
    // for the largest packet this engine can produce (up to 256 MiB each; larger on first need)
    const size_t maxw = host::max_packet_words(kind, n_inst, e->hs.n_ev(),
                                               std::max(host::max_segments(kind), host::max_note_segments(kind))) +
                        host::max_timed_param_words(kind, n_inst) +
                        host::max_timed_instrument_words(kind, n_inst, e->hs.voices);
    for (olfx_engine::Slot &sl : e->slot)
        if (!rc) rc = grow_slot(e, sl, olfx_engine::kCopyBytes / 4, false);
    if (maxw * 4 >= e->copy_bytes && maxw * 4 <= ((size_t)256 << 20))
        for (olfx_engine::Slot &sl : e->big)
            if (!rc) rc = grow_slot(e, sl, maxw, true);
    if (rc) {
        olfx_destroy(e);
        return rc;
    }
    *out = e;
    return OLFX_OK;
}

int olfx_destroy(olfx_engine *e) {
    if (!e) return OLFX_E_ARG;
    if (e->trace && e->tr_calls)
        std::fprintf(stderr, "olfx control trace (kind %d, %llu packets, mean us): fold %.2f slot-free %.2f "
                     "alloc %.2f coefficients %.2f events+deliver %.2f scatter %.2f\n", e->kind,
                     (unsigned long long)e->tr_calls, e->tr[0] / e->tr_calls, e->tr[1] / e->tr_calls,
                     e->tr[2] / e->tr_calls, e->tr[3] / e->tr_calls, e->tr[4] / e->tr_calls, e->tr[5] / e->tr_calls);
    (void)hipSetDevice(e->device);
    // the engine's own work only (its latest launch stream, its streams, its slots' markers): other
    // engines and the host application's kernels keep running
    if (wait_engine(e) != OLFX_OK) (void)hipDeviceSynchronize();
    e->each_slot([](olfx_engine::Slot &sl) {
        if (sl.h) (void)hipHostFree(sl.h);
        if (sl.d) (void)hipFree(sl.d);
        if (sl.copied) (void)hipEventDestroy(sl.copied);
        if (sl.consumed) (void)hipEventDestroy(sl.consumed);
    });
    if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
    if (e->dt_pre_tmp) (void)hipFree(e->dt_pre_tmp);
    if (e->tile_in) (void)hipFree(e->tile_in);
    if (e->tile_out) (void)hipFree(e->tile_out);
    if (e->d_mem) (void)hipFree(e->d_mem);
    if (e->h_in) (void)hipHostFree(e->h_in);
    if (e->h_out) (void)hipHostFree(e->h_out);
    if (e->d_in) (void)hipFree(e->d_in);
    if (e->d_out) (void)hipFree(e->d_out);
    if (e->mix_dev) (void)hipFree(e->mix_dev);
    if (e->sm_bank) (void)hipFree(e->sm_bank);
    if (e->mix_done) (void)hipEventDestroy(e->mix_done);
    if (e->switched) (void)hipEventDestroy(e->switched);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return OLFX_OK;
}

int olfx_reset(olfx_engine *e) {
    if (!e) return OLFX_E_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    if (const int rc = wait_engine(e)) return rc;               // the last block, engine-scoped
    return init_state(e);
}

// ---- parameters, control changes and note events: the host shadow's operations ----
int olfx_set_params(olfx_engine *e, uint32_t first, uint32_t count, uint32_t field0, uint32_t n_fields,
                    const float *values) {
    return e ? e->report(e->hs.set_range(first, count, field0, n_fields, values)) : OLFX_E_ARG;
}

int olfx_set_param_list(olfx_engine *e, uint32_t field, const uint32_t *inst, const float *values, uint32_t count) {
    return e ? e->report(e->hs.set_list(field, inst, values, count)) : OLFX_E_ARG;
}

int olfx_set_param(olfx_engine *e, uint32_t inst, uint32_t field, float value) {
    return olfx_set_params(e, inst, 1, field, 1, &value);
}

int olfx_set_member(olfx_engine *e, uint32_t inst, uint32_t field, float value) {
    return e ? e->report(e->hs.set_member(inst, field, value)) : OLFX_E_ARG;
}

int olfx_get_param(olfx_engine *e, uint32_t inst, uint32_t field, float *value) {
    if (!e || !value || inst >= e->n || field >= e->hs.n_params) return OLFX_E_ARG;
    *value = e->hs.params[(size_t)field * e->n + inst];
    return OLFX_OK;
}

int olfx_control(olfx_engine *e, const olfx_control_event *ev, uint32_t n) {
    return e ? e->report(e->hs.control(ev, n)) : OLFX_E_ARG;
}

int olfx_note_events(olfx_engine *e, const olfx_event *ev, uint32_t n) {
    return e ? e->report(e->hs.note_events(ev, n)) : OLFX_E_ARG;
}

int olfx_voice_events(olfx_engine *e, const olfx_voice_event *ev, uint32_t n) {
    return e ? e->report(e->hs.voice_events(ev, n)) : OLFX_E_ARG;
}

int olfx_timed_events(olfx_engine *e, const olfx_timed_event *ev, uint32_t n) {
    return e ? e->report(e->hs.timed_events(ev, n)) : OLFX_E_ARG;
}

int olfx_timed_notes(olfx_engine *e, const olfx_timed_note *ev, uint32_t n) {
    return e ? e->report(e->hs.timed_notes(ev, n)) : OLFX_E_ARG;
}

int olfx_timed_params(olfx_engine *e, const olfx_timed_param *rec, uint32_t n) {
    return e ? e->report(e->hs.timed_params(rec, n)) : OLFX_E_ARG;
}

int olfx_timed_control(olfx_engine *e, const struct olfx_timed_control *rec, uint32_t n) {
    return e ? e->report(e->hs.timed_control(rec, n)) : OLFX_E_ARG;
}

int olfx_timed_instrument_params(olfx_engine *e, const olfx_timed_param *rec, uint32_t n) {
    return e ? e->report(e->hs.timed_instrument_params(rec, n)) : OLFX_E_ARG;
}

int olfx_timed_instrument_control(olfx_engine *e, const struct olfx_timed_control *rec, uint32_t n) {
    return e ? e->report(e->hs.timed_instrument_control(rec, n)) : OLFX_E_ARG;
}

int olfx_synth_playing(olfx_engine *e, uint32_t inst, uint8_t *playing) {
    return e ? e->report(e->hs.synth_playing(inst, playing)) : OLFX_E_ARG;
}

int olfx_update(olfx_engine *e, uint32_t first, uint32_t count) {
    return e ? e->report(e->hs.update(first, count)) : OLFX_E_ARG;
}

int olfx_process(olfx_engine *e, const float *in, float *out, uint32_t n_frames, int io_flags, void *stream) {
    if (!e) return OLFX_E_ARG;
    if (n_frames == 0) return OLFX_OK;
    // (a meter without `out` runs its summary mode)
    const bool summary = !out && is_meter_kind(e->kind);
    if ((n_frames & 3u) || (!out && !summary) || (in_channels(e->kind) && !in))
        return e->fail(OLFX_E_ARG, "olfx_process: bad argument (n_frames=%u must be a multiple of 4)", n_frames);
    if (io_flags != OLFX_IO_DEVICE && io_flags != OLFX_IO_HOST)
        return e->fail(OLFX_E_ARG, "olfx_process: bad io_flags");
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;   // NULL = the HIP default (null) stream
    const size_t fin = (size_t)in_channels(e->kind) * n_frames * e->n;
    const size_t fout = summary ? 0 : (size_t)out_channels(e->kind) * n_frames * e->n;
    // a stream switch: this block's work (the control scatter included) after the previous launch
    int rc = order_after_last(e, s);
    if (rc) return rc;
    if (io_flags == OLFX_IO_HOST) {
        rc = ensure_staging(e, fin ? fin : 1, fout ? fout : 1);
        if (rc) return rc;
    }
    // the block's parameter changes and note events: asynchronous, O(changed)
    // One pass over all the frames -- unless timed events sit at more distinct frames than a launch takes
    // segments (host::Shadow::span: the voice kinds and the instrument kinds, no input): then a pass per run of
    // segments, each with its own packet, the state carrying between them as between run_frames' tiles.  A run
    // writes its frames of every output plane: the planes stay the whole call's distance apart.
    const bool host_io = io_flags == OLFX_IO_HOST;
    const float *const rin = host_io ? (fin ? e->d_in : nullptr) : in;
    float *const rout = host_io ? (summary ? nullptr : e->d_out) : out;
    for (uint32_t f0 = 0; f0 < n_frames;) {
        const uint32_t span = e->hs.span(n_frames - f0);
        VoiceArgs ev{};
        InstrumentTimed tp{};
        olfx_engine::Slot *sl = nullptr;
        rc = submit_control(e, s, &ev, &tp, &sl, span);
        if (rc) return rc;
        if (host_io && fin && f0 == 0) {
            std::memcpy(e->h_in, in, fin * 4);
            const hipError_t r = hipMemcpyAsync(e->d_in, e->h_in, fin * 4, hipMemcpyHostToDevice, s);
            if (r != hipSuccess) rc = e->hip_fail(r, "olfx_process: input copy");
        }
        if (!rc) rc = run_frames(e, rin, rout ? rout + (size_t)f0 * e->n : nullptr, span, n_frames, s, ev, tp);
        launched_on(e, s);
        // the slot is free again once whatever was queued on `s` (the scatter, the kernels) is done --
        // recorded on the error paths too, so a later block never overwrites a packet still being read
        if (sl) {
            const hipError_t r = slot_queued(e, sl, s);
            if (!rc && r != hipSuccess) rc = e->hip_fail(r, "hipEventRecord(consumed)");
        }
        if (rc) return rc;
        e->hs.advance(span);              // pending timed events count from the next launch
        f0 += span;
    }
    if (io_flags == OLFX_IO_HOST) {
        if (fout) HIPCHK(e, hipMemcpyAsync(e->h_out, e->d_out, fout * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(e, hipStreamSynchronize(s));
        if (fout) std::memcpy(out, e->h_out, fout * 4);
    }
    return OLFX_OK;
}

// ---- level meters: the state rows of a range of instances, on the host ----
int olfx_meter_read(olfx_engine *e, uint32_t first, uint32_t count, olfx_meter_level *levels) {
    if (!e) return OLFX_E_ARG;
    if (!is_meter_kind(e->kind)) return e->fail(OLFX_E_STATE, "olfx_meter_read: not a meter engine");
    if ((uint64_t)first + count > e->n || (count && !levels)) return e->fail(OLFX_E_ARG, "olfx_meter_read: range out of bounds");
    if (!count) return OLFX_OK;
    HIPCHK(e, hipSetDevice(e->device));
    if (const int rc = wait_engine(e)) return rc;               // this engine's queued blocks only
    const uint32_t ch = in_channels(e->kind);
    const size_t signals = (size_t)ch * e->n;
    std::vector<float> rows((size_t)MTS_N * ch * count);
    for (uint32_t f = 0; f < MTS_N; ++f)
        for (uint32_t c = 0; c < ch; ++c)
            HIPCHK(e, hipMemcpy(rows.data() + ((size_t)f * ch + c) * count, e->mt_state + f * signals + (size_t)c * e->n + first,
                                (size_t)count * 4, hipMemcpyDeviceToHost));
    auto row = [&](uint32_t f, uint32_t c, uint32_t k) { return rows[((size_t)f * ch + c) * count + k]; };
    for (uint32_t k = 0; k < count; ++k)
        for (uint32_t c = 0; c < ch; ++c)
            levels[(size_t)k * ch + c] = olfx_meter_level{row(MTS_RMS, c, k), row(MTS_PEAK, c, k), row(MTS_SUM, c, k),
                                                          row(MTS_COUNT, c, k), row(MTS_PEAK_COUNT, c, k)};
    return OLFX_OK;
}

// ---- voice buses: Polyvoice::Process / VoiceMap::Process (Polyvoice.h:28-33, VoiceMap.h:64-73) ----
int olfx_mix_config(olfx_engine *e, uint32_t n_buses, const uint32_t *offsets, const uint32_t *order) {
    if (!e) return OLFX_E_ARG;
    if (!is_voice_kind(e->kind)) return e->fail(OLFX_E_STATE, "olfx_mix_config: not a voice engine");
    std::vector<uint32_t> h;
    if (n_buses) {
        if (!offsets || offsets[0] != 0) return e->fail(OLFX_E_ARG, "olfx_mix_config: offsets must start at 0");
        for (uint32_t b = 0; b < n_buses; ++b)
            if (offsets[b + 1] < offsets[b])
                return e->fail(OLFX_E_ARG, "olfx_mix_config: offsets decrease at bus %u", b);
        const uint32_t len = offsets[n_buses];
        if (len > e->n)
            return e->fail(OLFX_E_ARG, "olfx_mix_config: %u entries for %u voices (each voice at most once)", len, e->n);
        if (len && !order) return e->fail(OLFX_E_ARG, "olfx_mix_config: null order");
        std::vector<uint8_t> seen(e->n, 0);
        for (uint32_t k = 0; k < len; ++k) {
            if (order[k] >= e->n)
                return e->fail(OLFX_E_ARG, "olfx_mix_config: order[%u] = %u out of range", k, order[k]);
            // listed twice, the reference would run the voice twice per frame (Polyvoice.h:28-33)
            if (seen[order[k]]++) return e->fail(OLFX_E_ARG, "olfx_mix_config: voice %u listed twice", order[k]);
        }
        h.assign(offsets, offsets + n_buses + 1);
        h.insert(h.end(), order, order + len);
    }
    HIPCHK(e, hipSetDevice(e->device));
    // the new lists first: a failed allocation leaves the current configuration in place
    uint32_t *fresh = nullptr;
    if (n_buses) {
        HIPCHK(e, hipMalloc((void **)&fresh, h.size() * 4));
        const hipError_t r = hipMemcpy(fresh, h.data(), h.size() * 4, hipMemcpyHostToDevice);
        if (r != hipSuccess) {
            (void)hipFree(fresh);
            return e->hip_fail(r, "olfx_mix_config upload");
        }
    }
    if (e->mix_dev) {   // the last mix launched (on any stream) may still read the old lists
        hipError_t r = e->mix_done ? hipEventSynchronize(e->mix_done) : hipSuccess;
        if (r == hipSuccess) r = hipFree(e->mix_dev);
        if (r != hipSuccess) {          // the current configuration stays; the new lists are dropped
            if (fresh) (void)hipFree(fresh);
            return e->hip_fail(r, "olfx_mix_config: releasing the previous lists");
        }
    }
    e->mix_dev = fresh;
    e->n_buses = n_buses;
    // buses that are contiguous voice runs in voice order, on multiples of 4 voices, take
    // voice_mix_v4 (float4 runs)
    e->mix_quad = 0;
    if (n_buses) {
        const uint32_t len = offsets[n_buses];
        bool quad = true;
        for (uint32_t k = 0; k < len && quad; ++k) quad = order[k] == k;
        for (uint32_t b = 0; b <= n_buses && quad; ++b) quad = (offsets[b] & 3u) == 0;
        e->mix_quad = quad ? 1u : 0u;
    }
    return OLFX_OK;
}

int olfx_mix(olfx_engine *e, const float *voice_out, float *bus_out, uint32_t n_frames, int io_flags, void *stream) {
    if (!e) return OLFX_E_ARG;
    if (!e->n_buses) return e->fail(OLFX_E_STATE, "olfx_mix: no buses (olfx_mix_config)");
    if (n_frames == 0) return OLFX_OK;
    if (!voice_out || !bus_out) return e->fail(OLFX_E_ARG, "olfx_mix: null buffer");
    if (io_flags != OLFX_IO_DEVICE && io_flags != OLFX_IO_HOST) return e->fail(OLFX_E_ARG, "olfx_mix: bad io_flags");
    HIPCHK(e, hipSetDevice(e->device));
    if (!e->mix_done) HIPCHK(e, hipEventCreateWithFlags(&e->mix_done, hipEventDisableTiming));
    hipStream_t s = (hipStream_t)stream;
    // a stream switch, as in olfx_process: the mix after the engine's previous launch, and the next
    // launch (on whichever stream) after the mix
    if (const int rc = order_after_last(e, s)) return rc;
    const bool host_io = io_flags == OLFX_IO_HOST;
    const size_t fin = (size_t)n_frames * e->n, fout = (size_t)n_frames * e->n_buses;
    if (host_io) {
        if (const int rc = ensure_staging(e, fin, fout)) return rc;
        std::memcpy(e->h_in, voice_out, fin * 4);
        std::memcpy(e->h_out, bus_out, fout * 4);
        HIPCHK(e, hipMemcpyAsync(e->d_in, e->h_in, fin * 4, hipMemcpyHostToDevice, s));
        HIPCHK(e, hipMemcpyAsync(e->d_out, e->h_out, fout * 4, hipMemcpyHostToDevice, s));
    }
    MixArgs a{};
    a.in = host_io ? e->d_in : voice_out;
    a.out = host_io ? e->d_out : bus_out;
    a.off = e->mix_dev;
    a.order = e->mix_dev + e->n_buses + 1;
    a.quad = e->mix_quad;
    a.n = e->n;
    a.n_buses = e->n_buses;
    a.n_frames = n_frames;
    const hipError_t r = launch_mix(a, s);
    if (r != hipSuccess) return e->hip_fail(r, "mix launch");
    HIPCHK(e, hipEventRecord(e->mix_done, s));
    if (host_io) {
        HIPCHK(e, hipMemcpyAsync(e->h_out, e->d_out, fout * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(e, hipStreamSynchronize(s));
        std::memcpy(bus_out, e->h_out, fout * 4);
    }
    launched_on(e, s);
    return OLFX_OK;
}

// ---- sample voices: the bank and each voice's Sample (validation and layout: host::Shadow) ----
int olfx_sample_bank(olfx_engine *e, uint32_t n_samples, const uint64_t *offsets, const float *pcm) {
    if (!e) return OLFX_E_ARG;
    host::BankPlan plan;
    if (const int rc = e->report(e->hs.bank_plan(n_samples, offsets, pcm, &plan))) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    // the new bank first: a failed allocation leaves the current one in place
    float *fresh = nullptr;
    if (plan.floats) {
        std::vector<float> h;
        try {
            h.assign((size_t)plan.floats, 0.f);        // aligned starts, zeroed gaps and tail
        } catch (const std::bad_alloc &) {
            return e->fail(OLFX_E_NOMEM, "olfx_sample_bank: host staging of %llu bytes", (unsigned long long)plan.floats * 4);
        }
        for (size_t k = 0; k < plan.len.size(); ++k)
            if (plan.len[k]) std::memcpy(h.data() + plan.base[k], pcm + offsets[k], (size_t)plan.len[k] * 4);
        hipError_t r = hipMalloc((void **)&fresh, (size_t)plan.floats * 4);
        if (r != hipSuccess)
            return e->fail(OLFX_E_NOMEM, "olfx_sample_bank: hipMalloc(%llu bytes): %s", (unsigned long long)plan.floats * 4,
                           hipGetErrorString(r));
        r = hipMemcpy(fresh, h.data(), (size_t)plan.floats * 4, hipMemcpyHostToDevice);
        if (r != hipSuccess) {
            (void)hipFree(fresh);
            return e->hip_fail(r, "olfx_sample_bank upload");
        }
    }
    // the blocks queued so far still read the old bank: this engine's work only, as olfx_reset
    if (const int rc = wait_engine(e)) {
        if (fresh) (void)hipFree(fresh);
        return rc;
    }
    if (e->sm_bank) (void)hipFree(e->sm_bank);
    e->sm_bank = fresh;
    e->sm_bank_bytes = plan.floats * 4;
    e->hs.bank_commit(std::move(plan));
    return OLFX_OK;
}

int olfx_sample_voices(olfx_engine *e, const olfx_sample_voice *recs, uint32_t n) {
    return e ? e->report(e->hs.sample_voices(recs, n)) : OLFX_E_ARG;
}

int olfx_drumkit_map(olfx_engine *e, const olfx_drumkit_voice *recs, uint32_t n) {
    return e ? e->report(e->hs.drumkit_map(recs, n)) : OLFX_E_ARG;
}

int olfx_sync(olfx_engine *e) {
    if (!e) return OLFX_E_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    return wait_engine(e);
}

void *olfx_stream(const olfx_engine *e) { return e ? (void *)e->stream : nullptr; }

uint32_t olfx_num_instances(const olfx_engine *e) { return e ? e->n : 0; }
int olfx_kind(const olfx_engine *e) { return e ? e->kind : 0; }
uint64_t olfx_frames_processed(const olfx_engine *e) { return e ? e->frames : 0; }
uint32_t olfx_num_buses(const olfx_engine *e) { return e ? e->n_buses : 0; }
uint32_t olfx_synth_voices(const olfx_engine *e) { return e ? e->hs.voices : 0; }

double olfx_algorithmic_bytes_per_frame(const olfx_engine *e) {
    // (a drum kit reads 4 B of sample per voice and frame on top of its row's figure)
    return e ? host::algorithmic_bytes_per_frame(e->kind) + (e->hs.kit() ? 4.0 * e->hs.voices : 0.0) : 0.0;
}
double olfx_algorithmic_read_bytes_per_frame(const olfx_engine *e) {
    return e ? host::algorithmic_read_bytes_per_frame(e->kind) + (e->hs.kit() ? 4.0 * e->hs.voices : 0.0) : 0.0;
}

const char *olfx_kernel_name(const olfx_engine *e) {
    if (!e) return "";
    // the standalone reverb's: the network of the last block (dattorro.hip dattorro_network)
    return e->hs.kd->kernel ? e->hs.kd->kernel : dattorro_network_name(e->dt_net);
}

int olfx_chorus_ring_free(const olfx_engine *e) {
    if (!e || e->kind != OLFX_KIND_CHORUS) return -1;
    return e->hs.ring_free_next() ? 1 : 0;
}

const char *olfx_last_error(const olfx_engine *e) {
    if (e) return e->err.c_str();
    std::lock_guard<std::mutex> lk(g_err_mu);
    static thread_local std::string copy;
    copy = g_err;
    return copy.c_str();
}

}  // extern "C"
