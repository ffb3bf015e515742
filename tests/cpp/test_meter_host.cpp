/*
 * tests/cpp/test_meter_host.cpp -- OLFX_KIND_METER and OLFX_KIND_METER_MONO in the engine's HIP-free host core
 * (ol_dsp_amd/csrc/olfx_host.h) on the CPU: the two rows (channels, fields, defaults, state bytes, the bytes-per-
 * frame figures), window 0 resolved against the rate in fp32, non-finite values refused with nothing changed, packets
 * of the changed instances only, what reset keeps and what it clears, and no control mapping.  Links olfx_host.cpp
 * directly (no libolfx.so, no GPU); built by tests/test_meter_host.py with its own build line.
 */
#include <limits>

#include "../../ol_dsp_amd/csrc/olfx_host.h"
#include "harness.h"

using namespace olfx;
using host::Shadow;

namespace {

constexpr int K2 = OLFX_KIND_METER, K1 = OLFX_KIND_METER_MONO;

uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

/* the next block's packet: (listed instances, records [MTC_N][m]) */
struct Packet {
    bool dense;
    std::vector<uint32_t> inst, window, hold;
};
Packet drain(Shadow &s) {
    const host::PacketPlan pl = s.plan(false);
    std::vector<uint32_t> buf(pl.words + 4);
    const size_t m = s.dirty_list.size();
    s.fill_records(pl, buf.data());
    Packet p{pl.dense, {}, {}, {}};
    for (size_t r = 0; r < m; ++r) {
        p.inst.push_back(pl.dense ? (uint32_t)r : buf[pl.o_inst + r]);
        p.window.push_back(buf[pl.o_val + MTC_WINDOW * m + r]);
        p.hold.push_back(buf[pl.o_val + MTC_HOLD * m + r]);
    }
    return p;
}

Shadow fresh(int kind, uint32_t n, float sr = 48000.f) {
    Shadow s;
    s.init(kind, n, sr);
    s.reset();
    return s;
}

}  // namespace

TEST(Meter, TheTwoRows) {
    EXPECT_EQ(OLFX_KIND_METER, 15);
    EXPECT_EQ(OLFX_KIND_METER_MONO, 16);
    EXPECT_EQ(OLFX_ABI_VERSION, 2);
    EXPECT_EQ(OLFX_MT_NPARAMS, 2);
    EXPECT_EQ(host::n_params_of(13), 0u);
    EXPECT_EQ(host::n_params_of(17), 0u);
    for (const int k : {K2, K1}) {
        const uint32_t ch = k == K2 ? 2u : 1u;
        EXPECT_EQ(host::n_params_of(k), 2u);
        EXPECT_EQ(host::in_channels(k), ch);
        EXPECT_EQ(host::out_channels(k), ch);
        EXPECT_TRUE(!host::takes_note_events(k) && !is_voice_kind(k) && !is_synth_kind(k) && is_meter_kind(k));
        EXPECT_EQ(std::string(host::kind_desc(k).kernel), std::string("meter_block_v1"));
        EXPECT_TRUE(!host::kind_desc(k).planes_32bit);
        /* five floats per channel, two coefficient words per instance */
        EXPECT_EQ(host::state_bytes(k, 1, 48000.f), (uint64_t)(5 * ch + 2) * 4);
        EXPECT_EQ(host::state_bytes(k, 65, 44100.f), (uint64_t)(5 * ch + 2) * 4 * 65);
        /* the envelope mode's figure: 4 B in + 4 B out per signal-frame; its read share is what summary mode moves */
        EXPECT_EQ(host::algorithmic_bytes_per_frame(k), 8.0 * ch);
        EXPECT_EQ(host::algorithmic_read_bytes_per_frame(k), 4.0 * ch);
        const host::Segments sg = host::coef_segments(k);
        EXPECT_EQ(sg.nseg, 1u);
        EXPECT_EQ(sg.words[0], (uint32_t)MTC_N);
        EXPECT_EQ(sg.total(), 2u);
        EXPECT_EQ(host::voice_segments(k).nseg, 0u);
        float p[OLFX_MT_NPARAMS] = {-1.f, -1.f};
        host::default_params(k, p);
        EXPECT_EQ(bits(p[OLFX_MT_WINDOW]), bits(0.0f));
        EXPECT_EQ(bits(p[OLFX_MT_PEAK_HOLD]), bits(96000.0f));
    }
    EXPECT_TRUE(!is_meter_kind(OLFX_KIND_DRUMKIT) && !is_meter_kind(13) && !is_meter_kind(0));
    EXPECT_EQ((int)MTS_N, 5);
}

TEST(Meter, WindowZeroIsTheRatesDefaultInFp32) {
    const struct { float sr; float window; } rates[] = {{44100.f, 0x1.d66666p+6f}, {48000.f, 128.f}, {96000.f, 256.f}};
    for (const auto &r : rates)
        for (const int k : {K2, K1}) {
            Shadow s = fresh(k, 3, r.sr);
            const Packet p = drain(s);                       /* the first block: every instance */
            EXPECT_TRUE(p.dense);
            EXPECT_EQ(p.inst.size(), (size_t)3);
            for (size_t i = 0; i < p.window.size(); ++i) {
                EXPECT_EQ(p.window[i], bits(r.window));
                EXPECT_EQ(p.hold[i], bits(96000.f));         /* the literal: it does not follow the rate */
            }
        }
    /* 117.6 is no whole number: no count ever equals it */
    EXPECT_TRUE(0x1.d66666p+6f != 117.f && 0x1.d66666p+6f != 118.f && 0x1.d66666p+6f == 44100.f / 375);
    /* any finite value goes through as it is: fractional, negative, tiny, huge, -0 (which is `window != 0` false) */
    uint32_t w[MTC_N];
    const float cases[] = {117.6f, -3.f, 1e-40f, 3e38f, 1.f};
    for (const float v : cases) {
        const float p[2] = {v, -7.5f};
        host::derive_meter(p, 48000.f, w);
        EXPECT_EQ(w[MTC_WINDOW], bits(v));
        EXPECT_EQ(w[MTC_HOLD], bits(-7.5f));
    }
    const float neg0[2] = {-0.f, 5.f};
    host::derive_meter(neg0, 96000.f, w);
    EXPECT_EQ(w[MTC_WINDOW], bits(256.f));
}

TEST(Meter, NonFiniteRefusedWithNothingChanged) {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (const int k : {K2, K1}) {
        Shadow s = fresh(k, 8);
        drain(s);
        const float ok[4] = {300.f, 117.6f, -2.f, 0.5f};
        EXPECT_EQ(s.set_range(2, 2, OLFX_MT_WINDOW, 2, ok), OLFX_OK);
        drain(s);
        const std::vector<float> before = s.params;
        for (const float bad : {nan, inf, -inf}) {
            for (const uint32_t field : {(uint32_t)OLFX_MT_WINDOW, (uint32_t)OLFX_MT_PEAK_HOLD}) {
                EXPECT_EQ(s.set_range(1, 1, field, 1, &bad), OLFX_E_ARG);
                EXPECT_TRUE(std::string(s.msg).find("non-finite") != std::string::npos);
                const float mixed[3] = {1.f, bad, 2.f};      /* one bad value refuses the whole call */
                EXPECT_EQ(s.set_range(0, 3, field, 1, mixed), OLFX_E_ARG);
                const uint32_t inst[2] = {4, 5};
                const float vals[2] = {64.f, bad};
                EXPECT_EQ(s.set_list(field, inst, vals, 2), OLFX_E_ARG);
                EXPECT_EQ(s.set_member(6, field, bad), OLFX_E_ARG);
            }
        }
        EXPECT_TRUE(s.params == before);
        EXPECT_TRUE(s.dirty_list.empty());
        /* out of range */
        const float one = 1.f;
        EXPECT_EQ(s.set_range(8, 1, OLFX_MT_WINDOW, 1, &one), OLFX_E_ARG);
        EXPECT_EQ(s.set_range(0, 1, OLFX_MT_NPARAMS, 1, &one), OLFX_E_ARG);
        EXPECT_TRUE(s.params == before && s.dirty_list.empty());
    }
}

TEST(Meter, PacketsOfTheChangedOnly) {
    Shadow s = fresh(K2, 200);
    EXPECT_EQ(drain(s).inst.size(), (size_t)200);
    EXPECT_TRUE(drain(s).inst.empty());                       /* nothing changed: nothing to send */
    EXPECT_EQ(s.plan(false).words, (size_t)0);
    EXPECT_EQ(s.set_range(7, 1, OLFX_MT_WINDOW, 1, std::vector<float>{300.f}.data()), OLFX_OK);
    const uint32_t inst[3] = {150, 7, 199};
    const float hold[3] = {5.f, 16.f, 256.f};
    EXPECT_EQ(s.set_list(OLFX_MT_PEAK_HOLD, inst, hold, 3), OLFX_OK);
    EXPECT_EQ(s.set_member(150, OLFX_MT_WINDOW, 0.f), OLFX_OK);       /* as olfx_set_param on this kind */
    const host::PacketPlan pl = s.plan(false);
    EXPECT_TRUE(!pl.dense);
    EXPECT_TRUE(pl.words <= 4 + 2 * 4 + 4);                   /* three instances: a list and two rows of three */
    const Packet p = drain(s);
    EXPECT_TRUE(p.inst == (std::vector<uint32_t>{7, 150, 199}));
    EXPECT_TRUE(p.window == (std::vector<uint32_t>{bits(300.f), bits(128.f), bits(128.f)}));
    EXPECT_TRUE(p.hold == (std::vector<uint32_t>{bits(16.f), bits(5.f), bits(256.f)}));
    EXPECT_TRUE(drain(s).inst.empty());
    /* olfx_update: the instances' records again, unchanged */
    EXPECT_EQ(s.update(7, 1), OLFX_OK);
    const Packet again = drain(s);
    EXPECT_TRUE(again.inst == (std::vector<uint32_t>{7}) && again.window[0] == bits(300.f) && again.hold[0] == bits(16.f));
    EXPECT_TRUE(host::max_packet_words(K2, 200) >= 200 * 3);
}

TEST(Meter, ResetKeepsTheParametersAndSendsThemAgain) {
    for (const int k : {K2, K1}) {
        Shadow s = fresh(k, 5, 44100.f);
        drain(s);
        const float w[2] = {3.f, 117.6f}, h[2] = {1000.f, 5.f};
        EXPECT_EQ(s.set_range(1, 2, OLFX_MT_WINDOW, 1, w), OLFX_OK);
        EXPECT_EQ(s.set_range(3, 2, OLFX_MT_PEAK_HOLD, 1, h), OLFX_OK);
        const std::vector<float> before = s.params;
        s.reset();                                            /* olfx_reset: the device arrays are zeroed */
        EXPECT_TRUE(s.params == before);
        const Packet p = drain(s);                            /* ... so every record goes out again */
        EXPECT_TRUE(p.dense);
        EXPECT_EQ(p.inst.size(), (size_t)5);
        EXPECT_TRUE(p.window == (std::vector<uint32_t>{bits(0x1.d66666p+6f), bits(3.f), bits(117.6f), bits(0x1.d66666p+6f),
                                                       bits(0x1.d66666p+6f)}));
        EXPECT_TRUE(p.hold == (std::vector<uint32_t>{bits(96000.f), bits(96000.f), bits(96000.f), bits(1000.f), bits(5.f)}));
        /* a pending change that the device never saw is not lost by a reset either */
        const float late = 64.f;
        EXPECT_EQ(s.set_range(0, 1, OLFX_MT_WINDOW, 1, &late), OLFX_OK);
        s.reset();
        EXPECT_EQ(drain(s).window[0], bits(64.f));
        /* a fresh shadow starts at the defaults */
        Shadow t = fresh(k, 5, 44100.f);
        EXPECT_TRUE(t.params == (std::vector<float>{0, 0, 0, 0, 0, 96000, 96000, 96000, 96000, 96000}));
    }
    /* the other kinds still go back to their defaults */
    Shadow r = fresh(OLFX_KIND_FXRACK, 2);
    const std::vector<float> defaults = r.params;
    const float fb = 0.25f;
    EXPECT_EQ(r.set_range(1, 1, OLFX_FR_DELAY_FEEDBACK, 1, &fb), OLFX_OK);
    r.reset();
    EXPECT_TRUE(r.params == defaults);
}

TEST(Meter, NoControlMapsToAMeter) {
    for (const int k : {K2, K1}) {
        uint32_t f = 77;
        float v = -1.f;
        for (int cc = 0; cc < 128; ++cc)
            for (const int src : {(int)OLFX_CTL_MIDI, (int)OLFX_CTL_HARDWARE})
                EXPECT_EQ(olfx_control_map(k, (uint8_t)cc, src, 64.f, &f, &v), OLFX_E_KIND);
        EXPECT_TRUE(f == 77 && v == -1.f);
        uint32_t f2[2];
        float v2[2];
        EXPECT_EQ(olfx_synth_control_map_at(k, 1, 7, OLFX_CTL_MIDI, 64.f, f2, v2), OLFX_E_KIND);
        Shadow s = fresh(k, 4);
        drain(s);
        const std::vector<float> before = s.params;
        const olfx_control_event ev{1u, 7, OLFX_CTL_MIDI, 0, 64.f};
        EXPECT_EQ(s.control(&ev, 1), OLFX_E_KIND);
        EXPECT_EQ(s.control(nullptr, 0), OLFX_E_KIND);
        EXPECT_TRUE(s.params == before && s.dirty_list.empty());
        const olfx_event note{0u, OLFX_EV_NOTE_ON, 60, 100, 0};
        EXPECT_EQ(s.note_events(&note, 1), OLFX_E_STATE);
    }
    /* the kinds with controls keep them */
    uint32_t f = 0;
    float v = 0.f;
    EXPECT_EQ(olfx_control_map(OLFX_KIND_FXRACK, 7, OLFX_CTL_MIDI, 64.f, &f, &v), OLFX_OK);
    EXPECT_EQ(f, (uint32_t)OLFX_FR_MASTER_VOLUME);
}

int main() { return run_all_tests(); }
