/*
 * tests/cpp/test_sampler_bank.cpp -- olfx::SamplerBank (include/olfx_fx.hpp) over the plain C ABI.
 * Without a GPU construction throws OLFX_E_NODEVICE (exit 2); with one a three-voice kit is played:
 * a triggered one-shot and a triggered loop sound, an untriggered voice and a voice whose sample was
 * taken away stay exactly 0, a refused record throws and changes nothing (exit 0).
 * Built and run by tests/test_sampler_host.py.
 */
#include <cstdio>
#include <string>
#include <vector>

#include "olfx_fx.hpp"

int main() {
    try {
        olfx::SamplerBank bank(4, 48000.f);
        int bad = 0;
        auto expect = [&](bool ok, const char *what) { if (!ok) { std::printf("FAILED: %s\n", what); ++bad; } };
        std::vector<float> kick(300, 0.5f), hat(9);
        for (size_t k = 0; k < hat.size(); ++k) hat[k] = k & 1 ? -0.4f : 0.4f;
        bank.SetBank({kick, hat});
        bank.SetSample(0, 0);
        bank.SetSample(1, 1, olfx::SamplerBank::PlayMode::Loop, 2, 7);
        bank.SetSample(2, 0);                       /* never triggered */
        bank.SetSample(3, 1);
        bank.SetSample(3, OLFX_NO_SAMPLE);          /* taken away again */
        bool threw = false;
        try { bank.SetSample(0, 2); } catch (const olfx::Error &e) { threw = e.code() == OLFX_E_ARG; }
        expect(threw, "sample index past the bank is refused");
        bank.NoteOn(0, 60, 100);
        bank.GateOn(1);
        bank.NoteOn(3, 60, 100);
        const uint32_t F = 512, n = 4;
        std::vector<float> y((size_t)F * n, 1.f);
        bank.Process(y.data(), F);
        bool on[4] = {false, false, false, false};
        for (uint32_t f = 0; f < F; ++f)
            for (uint32_t i = 0; i < n; ++i) on[i] = on[i] || y[(size_t)f * n + i] != 0.f;
        expect(on[0], "the one-shot sounds");
        expect(on[1], "the loop sounds after GateOn");
        expect(!on[2], "an untriggered voice is exactly 0");
        expect(!on[3], "a voice without a sample is exactly 0");
        expect(std::string(bank.kernel_name()) == "sampler_block_v1", "kernel name");
        std::printf("%d problems\n", bad);
        return bad ? 1 : 0;
    } catch (const olfx::Error &e) {
        std::printf("olfx::Error: %s\n", e.what());
        return e.code() == OLFX_E_NODEVICE ? 2 : 1;
    }
}
