/*
 * tests/cpp/test_synth_svf_bank.cpp -- olfx::SynthBank (include/olfx_fx.hpp) with kind =
 * OLFX_KIND_SYNTH_SVF over the plain C ABI.  Without a GPU construction throws OLFX_E_NODEVICE (exit 2,
 * never OLFX_E_KIND); with one the bank reports its kernel and voices and a block after a NoteOn is
 * audible on channel 0 of both instruments, on channel 1 of the one at topology 1 and all zeros on
 * channel 1 of the one at topology 0 (exit 0).  Built and run by tests/test_synth_svf_host.py.
 */
#include <cstdio>
#include <string>
#include <vector>

#include "olfx_fx.hpp"

int main() {
    try {
        olfx::SynthBank bank(2, 48000.f, 5, 256, 0, OLFX_KIND_SYNTH_SVF);
        int bad = 0;
        auto expect = [&](bool ok, const char *what) { if (!ok) { std::printf("FAILED: %s\n", what); ++bad; } };
        expect(bank.voices() == 5, "voices");
        expect(std::string(bank.kernel_name()) == "synth_svf_block_v1", "kernel name");
        expect(bank.get(0, OLFX_SY_RACK0 + OLFX_FR_TOPOLOGY) == 1.f, "topology defaults to 1");
        bank.SetRack(0, OLFX_FR_TOPOLOGY, 0.f);
        for (uint32_t i = 0; i < 2; ++i) {
            bank.SetRack(i, OLFX_FR_DELAY_TIME, 0.001f);
            bank.NoteOn(i, (uint8_t)(60 + i), 100);
        }
        const uint32_t F = 1024, n = 2;
        std::vector<float> y((size_t)2 * F * n, 7.f);
        bank.Process(y.data(), F);
        bool l0 = false, l1 = false, r0 = false, r1 = false;
        for (uint32_t f = 0; f < F; ++f) {
            l0 = l0 || y[(size_t)f * n] != 0.f;
            l1 = l1 || y[(size_t)f * n + 1] != 0.f;
            r0 = r0 || y[((size_t)F + f) * n] != 0.f;
            r1 = r1 || y[((size_t)F + f) * n + 1] != 0.f;
        }
        expect(l0 && l1, "both instruments are audible on channel 0");
        expect(r1, "topology 1: channel 1 is the reverb's");
        expect(!r0, "topology 0: channel 1 is 0.0f x master");
        std::printf("%d problems\n", bad);
        return bad ? 1 : 0;
    } catch (const olfx::Error &e) {
        std::printf("olfx::Error: %s\n", e.what());
        return e.code() == OLFX_E_NODEVICE ? 2 : 1;
    }
}
