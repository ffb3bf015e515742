/*
 * tests/cpp/test_sampler_host.cpp -- OLFX_KIND_VOICE_SAMPLE in the engine's HIP-free host core
 * (ol_dsp_amd/csrc/olfx_host.h) on the CPU: the kind tables, the event folding with the seek bit in
 * every order of NoteOn / NoteOff / GateOn / GateOff at one boundary, the bank's validation and
 * layout, the voice records' validation (a rejected call changes nothing), and the Sample words the
 * kernel reads.  Links olfx_host.cpp directly (no libolfx.so, no GPU); built by
 * tests/test_sampler_host.py with its own build line.
 */
#include "../../ol_dsp_amd/csrc/olfx_host.h"
#include "harness.h"

using namespace olfx;
using host::Shadow;

namespace {

constexpr int K = OLFX_KIND_VOICE_SAMPLE;

Shadow fresh(int kind, uint32_t n) {
    Shadow s;
    s.init(kind, n, 48000.f);
    s.reset();
    const host::PacketPlan pl = s.plan(false);
    std::vector<uint32_t> buf(pl.words);
    s.fill_records(pl, buf.data());
    return s;
}

std::vector<uint32_t> record(const Shadow &s, uint32_t i) {
    std::vector<uint32_t> w(host::coef_segments(s.kind).total());
    s.derive_record(i, w.data());
    return w;
}

olfx_voice_event vev(uint32_t inst, uint8_t type, uint8_t note = 60, float value = 0.f) {
    return olfx_voice_event{inst, type, note, 100, 0, value};
}

/* a bank of the given lengths into the shadow, as olfx_sample_bank does after its upload */
int set_bank(Shadow &s, const std::vector<uint64_t> &lens) {
    std::vector<uint64_t> off(lens.size() + 1, 0);
    for (size_t k = 0; k < lens.size(); ++k) off[k + 1] = off[k] + lens[k];
    std::vector<float> pcm((size_t)off.back() + 1, 0.25f);
    host::BankPlan plan;
    const int rc = s.bank_plan((uint32_t)lens.size(), off.data(), pcm.data(), &plan);
    if (rc == OLFX_OK) s.bank_commit(std::move(plan));
    return rc;
}

olfx_sample_voice rec(uint32_t inst, uint32_t sample, uint32_t mode = 0, uint64_t ls = 0, uint64_t le = 0) {
    return olfx_sample_voice{inst, sample, mode, 0, ls, le};
}

}  // namespace

TEST(Sampler, TablesAreTheVoices) {
    EXPECT_EQ(OLFX_KIND_VOICE_SAMPLE, 10);
    EXPECT_EQ(host::n_params_of(9), 0u);            /* 9 stays a kind nobody has (tests/test_platerack_host.py) */
    EXPECT_EQ(OLFX_ABI_VERSION, 2);
    EXPECT_TRUE(is_voice_kind(K));
    EXPECT_EQ(host::n_params_of(K), 16u);
    EXPECT_EQ(host::in_channels(K), 0u);
    EXPECT_EQ(host::out_channels(K), 1u);
    float p[OLFX_VC_NPARAMS], q[OLFX_VC_NPARAMS];
    host::default_params(K, p);
    host::default_params(OLFX_KIND_VOICE, q);
    EXPECT_TRUE(std::memcmp(p, q, sizeof p) == 0);
    /* state: the voice's words and the Sample's; the bank is not state */
    EXPECT_EQ(host::state_bytes(K, 1, 48000.f), host::state_bytes(OLFX_KIND_VOICE, 1, 48000.f) + SMC_N * 4u);
    EXPECT_EQ(host::algorithmic_bytes_per_frame(K), 8.0);
    EXPECT_EQ(host::algorithmic_read_bytes_per_frame(K), 4.0);
    const host::Segments sg = host::coef_segments(K);
    EXPECT_EQ(sg.nseg, 2u);
    EXPECT_EQ(sg.words[0], (uint32_t)VCC_N);
    EXPECT_EQ(sg.words[1], (uint32_t)SMC_N);
    /* the voice part of the record is the Svf voice's, word for word */
    Shadow a = fresh(K, 3), b = fresh(OLFX_KIND_VOICE, 3);
    const float v[2] = {1234.5f, 0.6f};
    EXPECT_EQ(a.set_range(1, 1, OLFX_VC_FILTER_CUTOFF, 2, v), OLFX_OK);
    EXPECT_EQ(b.set_range(1, 1, OLFX_VC_FILTER_CUTOFF, 2, v), OLFX_OK);
    for (uint32_t i = 0; i < 3; ++i) {
        const std::vector<uint32_t> ra = record(a, i), rb = record(b, i);
        EXPECT_TRUE(std::memcmp(ra.data(), rb.data(), VCC_N * 4) == 0);
    }
}

TEST(Sampler, ControlMapIsTheVoices) {
    for (int source = 0; source < 2; ++source)
        for (int cc = 0; cc < 128; ++cc) {
            uint32_t f1 = 77, f2 = 77;
            float v1 = -1.f, v2 = -1.f;
            const float value = source == OLFX_CTL_MIDI ? 93.f : 0.37f;
            const int r1 = olfx_control_map(K, (uint8_t)cc, source, value, &f1, &v1);
            const int r2 = olfx_control_map(OLFX_KIND_VOICE, (uint8_t)cc, source, value, &f2, &v2);
            EXPECT_EQ(r1, r2);
            EXPECT_EQ(f1, f2);
            EXPECT_TRUE(std::memcmp(&v1, &v2, 4) == 0);
        }
    /* olfx_set_member: the pre-Init semantics of the voices */
    Shadow s = fresh(K, 2);
    EXPECT_EQ(s.set_member(0, OLFX_VC_FILTER_RESONANCE, 0.4f), OLFX_OK);
    EXPECT_EQ((int)s.configured[0], 0);
    EXPECT_EQ(s.update(0, 1), OLFX_OK);
    EXPECT_EQ(s.set_member(0, OLFX_VC_FILTER_RESONANCE, 0.5f), OLFX_E_STATE);
    EXPECT_EQ(s.set_member(0, OLFX_VC_FILTER_CUTOFF, 500.f), OLFX_OK);
}

/* Every order of the four gate calls at one boundary (4! = 24), every ordered pair and every single
   call: the record is what the reference's in-order application leaves.  Model: gate / playing follow
   the last call, NoteOn retriggers and sets the pitch, NoteOn / GateOn seek to 0. */
TEST(Sampler, FoldingWithTheSeekBit) {
    const uint8_t types[4] = {OLFX_EV_NOTE_ON, OLFX_EV_NOTE_OFF, OLFX_EV_GATE_ON, OLFX_EV_GATE_OFF};
    std::vector<std::vector<uint8_t>> seqs;
    for (int a = 0; a < 4; ++a) {
        seqs.push_back({types[a]});
        for (int b = 0; b < 4; ++b) {
            seqs.push_back({types[a], types[b]});
            for (int c = 0; c < 4; ++c)
                for (int d = 0; d < 4; ++d)
                    if (a != b && a != c && a != d && b != c && b != d && c != d)
                        seqs.push_back({types[a], types[b], types[c], types[d]});
        }
    }
    EXPECT_EQ(seqs.size(), (size_t)(4 + 16 + 24));
    for (const auto &seq : seqs) {
        Shadow s = fresh(K, 70);
        std::vector<olfx_voice_event> evs;
        bool gate_on = false, retrig = false, seek = false, freq = false;
        for (const uint8_t t : seq) {
            evs.push_back(vev(65, t, 72));
            if (t == OLFX_EV_NOTE_ON) { gate_on = true; retrig = true; seek = true; freq = true; }
            else if (t == OLFX_EV_GATE_ON) { gate_on = true; seek = true; }
            else gate_on = false;
        }
        EXPECT_EQ(s.voice_events(evs.data(), (uint32_t)evs.size()), OLFX_OK);
        s.fold_events();
        EXPECT_EQ(s.folded.size(), (size_t)1);
        const host::Folded &r = s.folded[0];
        EXPECT_EQ(r.inst, 65u);
        const uint32_t want = VEV_GATE_SET | (gate_on ? VEV_GATE_ON : 0u) | (retrig ? VEV_RETRIGGER : 0u) |
                              (seek ? VEV_SEEK : 0u) | (freq ? VEV_FREQ : 0u);
        EXPECT_EQ(r.op, want);
    }
    /* NoteOn then NoteOff: cursor 0, paused, envelopes retriggered */
    {
        Shadow s = fresh(K, 4);
        const olfx_voice_event e[2] = {vev(2, OLFX_EV_NOTE_ON), vev(2, OLFX_EV_NOTE_OFF)};
        EXPECT_EQ(s.voice_events(e, 2), OLFX_OK);
        s.fold_events();
        EXPECT_EQ(s.folded[0].op, (uint32_t)(VEV_GATE_SET | VEV_RETRIGGER | VEV_SEEK | VEV_FREQ));
    }
    /* SetFrequency is accepted and carries no seek */
    {
        Shadow s = fresh(K, 4);
        const olfx_voice_event e = vev(1, OLFX_EV_SET_FREQUENCY, 0, 220.f);
        EXPECT_EQ(s.voice_events(&e, 1), OLFX_OK);
        s.fold_events();
        EXPECT_EQ(s.folded[0].op, (uint32_t)VEV_FREQ);
    }
    /* the other voice kinds' records carry no seek bit: their packets are unchanged */
    {
        Shadow s = fresh(OLFX_KIND_VOICE, 4);
        const olfx_voice_event e[2] = {vev(0, OLFX_EV_NOTE_ON), vev(1, OLFX_EV_GATE_ON)};
        EXPECT_EQ(s.voice_events(e, 2), OLFX_OK);
        s.fold_events();
        EXPECT_EQ(s.folded[0].op & VEV_SEEK, 0u);
        EXPECT_EQ(s.folded[1].op & VEV_SEEK, 0u);
    }
}

TEST(Sampler, BankValidationAndLayout) {
    Shadow s = fresh(K, 4);
    host::BankPlan plan;
    std::vector<float> pcm(4096, 0.f);
    const uint64_t ok[4] = {0, 1, 66, 200};
    EXPECT_EQ(s.bank_plan(3, ok, pcm.data(), &plan), OLFX_OK);
    /* starts on multiples of the fetch width, the tail padded by one more */
    EXPECT_EQ(plan.base.size(), (size_t)3);
    EXPECT_EQ(plan.base[0], 0u);
    EXPECT_EQ(plan.base[1], 64u);
    EXPECT_EQ(plan.base[2], 192u);
    EXPECT_EQ(plan.len[0], 1u);
    EXPECT_EQ(plan.len[1], 65u);
    EXPECT_EQ(plan.len[2], 134u);
    EXPECT_EQ(plan.floats, (uint64_t)(192 + 192 + 64));
    for (size_t k = 0; k < 3; ++k) {
        EXPECT_EQ(plan.base[k] % kSmAlign, 0u);
        EXPECT_TRUE((uint64_t)plan.base[k] + plan.len[k] + kSmAlign <= plan.floats);
    }
    /* planning changed nothing */
    EXPECT_EQ(s.bank.len.size(), (size_t)0);
    /* refused: offsets not starting at 0, non-monotone offsets, null arrays, not a sampler engine */
    const uint64_t from1[3] = {1, 2, 3}, down[4] = {0, 10, 5, 20};
    EXPECT_EQ(s.bank_plan(2, from1, pcm.data(), &plan), OLFX_E_ARG);
    EXPECT_EQ(s.bank_plan(3, down, pcm.data(), &plan), OLFX_E_ARG);
    EXPECT_EQ(s.bank_plan(3, nullptr, pcm.data(), &plan), OLFX_E_ARG);
    EXPECT_EQ(s.bank_plan(3, ok, nullptr, &plan), OLFX_E_ARG);
    const uint64_t huge[2] = {0, 0xFFFFFFFFull};
    EXPECT_EQ(s.bank_plan(1, huge, pcm.data(), &plan), OLFX_E_ARG);
    const uint64_t big[2] = {0, (1ull << 30)};            /* past the 32-bit byte offsets of the fetch */
    EXPECT_EQ(s.bank_plan(1, big, pcm.data(), &plan), OLFX_E_ARG);
    EXPECT_TRUE(std::strlen(s.msg) > 0);
    Shadow v = fresh(OLFX_KIND_VOICE, 4);
    EXPECT_EQ(v.bank_plan(3, ok, pcm.data(), &plan), OLFX_E_STATE);
    /* n_samples = 0: no bank */
    EXPECT_EQ(s.bank_plan(0, nullptr, nullptr, &plan), OLFX_OK);
    EXPECT_EQ(plan.floats, (uint64_t)0);
    /* empty samples are allowed */
    const uint64_t empty[3] = {0, 0, 5};
    EXPECT_EQ(s.bank_plan(2, empty, pcm.data(), &plan), OLFX_OK);
    EXPECT_EQ(plan.len[0], 0u);
    EXPECT_EQ(plan.len[1], 5u);
}

TEST(Sampler, VoiceRecordsValidationAndWords) {
    Shadow s = fresh(K, 6);
    EXPECT_EQ(set_bank(s, {5, 100, 7}), OLFX_OK);
    /* the bank made every voice dirty; deliver */
    {
        const host::PacketPlan pl = s.plan(false);
        std::vector<uint32_t> buf(pl.words);
        s.fill_records(pl, buf.data());
    }
    const olfx_sample_voice good[3] = {rec(0, 1, OLFX_SAMPLE_LOOP, 10, 90), rec(3, 0), rec(5, 2, OLFX_SAMPLE_LOOP, 9, 0)};
    EXPECT_EQ(s.sample_voices(good, 3), OLFX_OK);
    EXPECT_EQ(s.dirty_list.size(), (size_t)3);
    {
        const std::vector<uint32_t> w = record(s, 0);
        const uint32_t *m = w.data() + VCC_N;
        EXPECT_EQ(m[SMC_BASE], 64u);
        EXPECT_EQ(m[SMC_LEN], 100u);
        EXPECT_EQ(m[SMC_LS], 10u);
        EXPECT_EQ(m[SMC_LE], 90u);
        EXPECT_EQ(m[SMC_MODE] & 1u, 1u);
    }
    {
        /* loop_start past the sample: Seek puts the cursor at the end */
        const std::vector<uint32_t> w = record(s, 5);
        const uint32_t *m = w.data() + VCC_N;
        EXPECT_EQ(m[SMC_LEN], 7u);
        EXPECT_EQ(m[SMC_LS], 7u);
        EXPECT_EQ(m[SMC_LE], 0u);
    }
    {
        /* unassigned: nothing to read */
        const std::vector<uint32_t> w = record(s, 1);
        EXPECT_EQ(w[VCC_N + SMC_LEN], 0u);
        EXPECT_EQ(w[VCC_N + SMC_BASE], 0u);
    }
    /* a loop end at or past the sample's end can never fire: delivered as none */
    const olfx_sample_voice past = rec(0, 1, OLFX_SAMPLE_LOOP, 10, 100);
    const uint32_t gen0 = s.samples[0].gen;
    EXPECT_EQ(s.sample_voices(&past, 1), OLFX_OK);
    EXPECT_EQ(record(s, 0)[VCC_N + SMC_LE], 0u);
    /* the same index with other loop points keeps the Sample object (no seek); another index is a fresh one */
    EXPECT_EQ(s.samples[0].gen, gen0);
    const olfx_sample_voice other = rec(0, 2), none = rec(0, OLFX_NO_SAMPLE);
    EXPECT_EQ(s.sample_voices(&other, 1), OLFX_OK);
    EXPECT_EQ(s.samples[0].gen, gen0 + 1);
    EXPECT_EQ(s.sample_voices(&none, 1), OLFX_OK);
    EXPECT_EQ(s.samples[0].gen, gen0 + 2);
    EXPECT_EQ(record(s, 0)[VCC_N + SMC_LEN], 0u);

    /* refused calls change nothing: index >= n_samples, bad mode, voice out of range -- each after a
       valid record in the same call */
    const std::vector<host::SampleAsg> before = s.samples;
    {
        const host::PacketPlan pl = s.plan(false);
        std::vector<uint32_t> buf(pl.words);
        s.fill_records(pl, buf.data());
    }
    const olfx_sample_voice bad_index[2] = {rec(1, 0), rec(2, 3)};
    const olfx_sample_voice bad_mode[2] = {rec(1, 0), rec(2, 1, 2)};
    const olfx_sample_voice bad_voice[2] = {rec(1, 0), rec(6, 1)};
    EXPECT_EQ(s.sample_voices(bad_index, 2), OLFX_E_ARG);
    EXPECT_EQ(s.sample_voices(bad_mode, 2), OLFX_E_ARG);
    EXPECT_EQ(s.sample_voices(bad_voice, 2), OLFX_E_ARG);
    EXPECT_EQ(s.sample_voices(nullptr, 2), OLFX_E_ARG);
    EXPECT_EQ(s.dirty_list.size(), (size_t)0);
    for (size_t i = 0; i < before.size(); ++i) {
        EXPECT_EQ(s.samples[i].sample, before[i].sample);
        EXPECT_EQ(s.samples[i].gen, before[i].gen);
    }
    Shadow v = fresh(OLFX_KIND_VOICE, 4);
    EXPECT_EQ(v.sample_voices(good, 1), OLFX_E_STATE);
}

TEST(Sampler, BankReplacementAndReset) {
    Shadow s = fresh(K, 4);
    EXPECT_EQ(set_bank(s, {5, 100, 7}), OLFX_OK);
    const olfx_sample_voice r[3] = {rec(0, 0), rec(1, 2, OLFX_SAMPLE_LOOP, 1, 3), rec(2, 1)};
    EXPECT_EQ(s.sample_voices(r, 3), OLFX_OK);
    const uint32_t g0 = s.samples[0].gen, g1 = s.samples[1].gen, g3 = s.samples[3].gen;
    /* fewer samples: index 2 is gone -> unassigned; the others stay; every Sample is fresh */
    EXPECT_EQ(set_bank(s, {9, 30}), OLFX_OK);
    EXPECT_EQ(s.samples[0].sample, 0u);
    EXPECT_EQ(s.samples[2].sample, 1u);
    EXPECT_EQ(s.samples[1].sample, (uint32_t)OLFX_NO_SAMPLE);
    EXPECT_TRUE(s.samples[0].gen != g0 && s.samples[1].gen != g1 && s.samples[3].gen != g3);
    EXPECT_EQ(s.dirty_list.size(), (size_t)4);
    EXPECT_EQ(record(s, 0)[VCC_N + SMC_LEN], 9u);
    EXPECT_EQ(record(s, 2)[VCC_N + SMC_LEN], 30u);
    EXPECT_EQ(record(s, 2)[VCC_N + SMC_BASE], 64u);
    /* reset keeps the bank and the assignments (configuration, like the voice buses) */
    s.reset();
    EXPECT_EQ(s.bank.len.size(), (size_t)2);
    EXPECT_EQ(s.samples[2].sample, 1u);
    EXPECT_EQ(record(s, 2)[VCC_N + SMC_LEN], 30u);
    EXPECT_EQ(s.dirty_list.size(), (size_t)4);
    /* n_samples = 0 removes the bank: every voice unassigned */
    EXPECT_EQ(set_bank(s, {}), OLFX_OK);
    for (uint32_t i = 0; i < 4; ++i) EXPECT_EQ(s.samples[i].sample, (uint32_t)OLFX_NO_SAMPLE);
    /* the largest packet holds every voice's record, Sample words included */
    EXPECT_TRUE(host::max_packet_words(K, 4) >= (size_t)4 * (VCC_N + SMC_N));
}

int main() { return run_all_tests(); }
