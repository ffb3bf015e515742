/*
 * tests/cpp/test_ringfree_host.cpp -- the chorus kind's kernel switch in the HIP-free host core
 * (ol_dsp_amd/csrc/olfx_host.h RingFree, Shadow::fill_records / ring_free_next) on the CPU: the
 * countdown after a pitch or window change, sets of the same value, sets before the first frame,
 * reset, and the geometry of the deeper x ring.  Links olfx_host.cpp directly (no library, no GPU).
 */
#include "../../ol_dsp_amd/csrc/olfx_host.h"
#include "harness.h"

using namespace olfx;
using host::Shadow;

namespace {

/* what the engine does with a block: deliver the dirty records, run the frames */
struct Block { bool ring_free, materialise; };
Block block(Shadow &s, uint32_t n_frames) {
    Block b{};
    if (!s.dirty_list.empty()) {
        const host::PacketPlan pl = s.plan(false);
        std::vector<uint32_t> buf(pl.words);
        s.fill_records(pl, buf.data());
    }
    b.materialise = s.rf_materialise;
    s.rf_materialise = false;
    b.ring_free = s.rf.active();
    s.rf.advance(n_frames);
    return b;
}

Shadow chorus(uint32_t n = 8) {
    Shadow s;
    s.init(OLFX_KIND_CHORUS, n, 48000.f);
    s.reset();
    return s;
}

void set(Shadow &s, uint32_t inst, uint32_t field, float v) { EXPECT_EQ(s.set_range(inst, 1, field, 1, &v), OLFX_OK); }

}  // namespace

TEST(RingFree, Geometry) {
    EXPECT_EQ(host::chorus_history(48000.f), 1154u);
    EXPECT_EQ(host::chorus_x_size(48000.f), 2048u);
    uint32_t ps, cs;
    host::chorus_sizes(48000.f, &ps, &cs);
    EXPECT_EQ(ps, 512u);                    /* the pitch-shift kind's and the chain's ring, and the clamp 510 */
    EXPECT_EQ(cs, 2048u);
    for (float sr : {8000.f, 44100.f, 48000.f, 88200.f, 96000.f, 192000.f, 384000.f}) {
        host::chorus_sizes(sr, &ps, &cs);
        const uint32_t x = host::chorus_x_size(sr);
        EXPECT_TRUE((x & (x - 1)) == 0);
        EXPECT_TRUE(x >= host::chorus_history(sr) - 2 + (ps - 2) + 64);
        EXPECT_TRUE(host::chorus_history(sr) <= cs);
    }
}

TEST(RingFree, SetsBeforeTheFirstFrameDoNotCount) {
    Shadow s = chorus();
    EXPECT_TRUE(s.ring_free_next());
    set(s, 3, OLFX_CH_PITCH, 2.0f);
    set(s, 4, OLFX_CH_WINDOW, 7.0f);
    EXPECT_TRUE(s.ring_free_next());
    const Block b = block(s, 256);
    EXPECT_TRUE(b.ring_free && !b.materialise);
    EXPECT_TRUE(s.ring_free_next());
}

TEST(RingFree, CountdownAfterAPitchChange) {
    Shadow s = chorus();
    EXPECT_TRUE(block(s, 256).ring_free);
    set(s, 2, OLFX_CH_PITCH, 1.5f);
    EXPECT_TRUE(!s.ring_free_next());                   /* pending: the next block would run the ring kernel */
    Block b = block(s, 256);
    EXPECT_TRUE(!b.ring_free && b.materialise);
    /* 1,154 frames of history: 256-frame blocks 2..5 after the change still run the ring kernel */
    for (int k = 0; k < 4; ++k) {
        b = block(s, 256);
        EXPECT_TRUE(!b.ring_free && !b.materialise);
    }
    EXPECT_TRUE(s.ring_free_next());                    /* 1,280 >= 1,154 */
    b = block(s, 256);
    EXPECT_TRUE(b.ring_free && !b.materialise);
    /* the count is in frames, not blocks */
    set(s, 2, OLFX_CH_WINDOW, 9.0f);
    EXPECT_TRUE(block(s, 1152).materialise);
    EXPECT_TRUE(!s.ring_free_next());
    EXPECT_TRUE(!block(s, 4).ring_free);                /* 1,152 < 1,154 */
    EXPECT_TRUE(block(s, 4).ring_free);                 /* 1,156 */
}

TEST(RingFree, AChangeInRingModeRestartsTheCountWithoutMaterialising) {
    Shadow s = chorus();
    block(s, 256);
    set(s, 0, OLFX_CH_PITCH, 1.0f);
    EXPECT_TRUE(block(s, 256).materialise);
    set(s, 0, OLFX_CH_PITCH, 2.0f);
    Block b = block(s, 256);
    EXPECT_TRUE(!b.ring_free && !b.materialise);        /* the ring is current: nothing to fill */
    for (int k = 0; k < 4; ++k) EXPECT_TRUE(!block(s, 256).ring_free);
    EXPECT_TRUE(block(s, 256).ring_free);
}

TEST(RingFree, OnlyPitchAndWindowWordsCount) {
    Shadow s = chorus();
    block(s, 256);
    float cur = s.params[(size_t)OLFX_CH_PITCH * s.n + 5];
    set(s, 5, OLFX_CH_PITCH, cur);                      /* the same value: no change */
    set(s, 5, OLFX_CH_DEPTH, 0.9f);
    set(s, 5, OLFX_CH_RATE, 0.3f);
    set(s, 5, OLFX_CH_MIX, 0.1f);
    set(s, 5, OLFX_CH_CUTOFF, 0.2f);
    set(s, 5, OLFX_CH_Q, 0.2f);
    set(s, 5, OLFX_CH_PHASE, 0.7f);
    EXPECT_TRUE(s.ring_free_next());
    Block b = block(s, 256);
    EXPECT_TRUE(b.ring_free && !b.materialise);
    /* values the setter clamps to the same word are the same coefficient */
    set(s, 5, OLFX_CH_PITCH, 3.0f);
    EXPECT_TRUE(block(s, 2048).materialise);
    EXPECT_TRUE(s.ring_free_next());
    set(s, 5, OLFX_CH_PITCH, 7.0f);                     /* clamped to 3 */
    EXPECT_TRUE(s.ring_free_next());
    b = block(s, 256);
    EXPECT_TRUE(b.ring_free && !b.materialise);
}

TEST(RingFree, ResetReturnsToRingFree) {
    Shadow s = chorus();
    block(s, 256);
    set(s, 1, OLFX_CH_PITCH, 2.5f);
    EXPECT_TRUE(block(s, 256).materialise);
    EXPECT_TRUE(!s.ring_free_next());
    s.reset();
    EXPECT_TRUE(s.ring_free_next());
    set(s, 1, OLFX_CH_PITCH, 2.5f);                     /* before the first frame again */
    const Block b = block(s, 256);
    EXPECT_TRUE(b.ring_free && !b.materialise);
}

TEST(RingFree, OtherKindsHaveNoSwitch) {
    Shadow s;
    s.init(OLFX_KIND_PITCHSHIFT, 4, 48000.f);
    s.reset();
    EXPECT_TRUE(!s.ring_free_next());
    EXPECT_TRUE(s.pitch_sent.empty());
    float v = 2.0f;
    EXPECT_EQ(s.set_range(0, 1, OLFX_PS_SHIFT, 1, &v), OLFX_OK);
    const host::PacketPlan pl = s.plan(false);
    std::vector<uint32_t> buf(pl.words);
    s.fill_records(pl, buf.data());
    EXPECT_TRUE(!s.rf_materialise);
}

int main() { return run_all_tests(); }
