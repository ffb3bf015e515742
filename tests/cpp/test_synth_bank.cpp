/*
 * tests/cpp/test_synth_bank.cpp -- olfx::SynthBank (include/olfx_fx.hpp) over the plain C ABI.  Without
 * a GPU construction throws OLFX_E_NODEVICE (exit 2); with one the Polyvoice calls move Playing() as
 * the rule says, a control change lands in both of its fields, and a block after a NoteOn is audible
 * on both channels for the instrument that plays and silent for the one that does not (exit 0).
 * Built and run by tests/test_synth_host.py.
 */
#include <cstdio>
#include <string>
#include <vector>

#include "olfx_fx.hpp"

int main() {
    try {
        olfx::SynthBank bank(2, 48000.f, 3);
        int bad = 0;
        auto expect = [&](bool ok, const char *what) { if (!ok) { std::printf("FAILED: %s\n", what); ++bad; } };
        expect(bank.voices() == 3, "voices");
        expect(std::string(bank.kernel_name()) == "synth_block_v1", "kernel name");
        expect(bank.get(0, OLFX_SY_RACK0 + OLFX_FR_TOPOLOGY) == 1.f, "topology defaults to 1");
        bank.NoteOn(1, 60, 100);
        bank.NoteOn(1, 64, 100);
        bank.NoteOff(1, 60, 0);
        bank.NoteOn(1, 67, 100);
        bank.NoteOn(1, 70, 100);
        bank.NoteOn(1, 72, 100);                              /* no voice free: dropped */
        expect((bank.Playing(1) == std::vector<uint8_t>{67, 64, 70}), "Playing() after the rule");
        expect((bank.Playing(0) == std::vector<uint8_t>{0, 0, 0}), "the other instrument is untouched");
        bank.UpdateMidiControl(1, 41, 100);                   /* CC_FILTER_CUTOFF: the voices and filter_fx */
        expect(bank.get(1, OLFX_SY_VOICE0 + OLFX_VC_FILTER_CUTOFF) > 0.f, "CC 41 -> the voice filter");
        expect(bank.get(1, OLFX_SY_RACK0 + OLFX_FR_FILTER_CUTOFF) < 20000.f, "CC 41 -> filter_fx");
        bank.SetRack(1, OLFX_FR_DELAY_TIME, 0.001f);
        const uint32_t F = 1024, n = 2;
        std::vector<float> y((size_t)2 * F * n, 0.f);
        bank.Process(y.data(), F);
        bool l0 = false, l1 = false, r0 = false, r1 = false;
        for (uint32_t f = 0; f < F; ++f) {
            l0 = l0 || y[(size_t)f * n] != 0.f;
            l1 = l1 || y[(size_t)f * n + 1] != 0.f;
            r0 = r0 || y[((size_t)F + f) * n] != 0.f;
            r1 = r1 || y[((size_t)F + f) * n + 1] != 0.f;
        }
        expect(l1 && r1, "the playing instrument is audible on both channels");
        expect(!l0 && !r0, "the idle instrument is silent");
        bank.reset();
        expect((bank.Playing(1) == std::vector<uint8_t>{0, 0, 0}), "reset clears Playing()");
        std::printf("%d problems\n", bad);
        return bad ? 1 : 0;
    } catch (const olfx::Error &e) {
        std::printf("olfx::Error: %s\n", e.what());
        return e.code() == OLFX_E_NODEVICE ? 2 : 1;
    }
}
