/*
 * tests/cpp/test_platerack_bank.cpp -- olfx::PlateRackBank (include/olfx_fx.hpp) over the plain C
 * ABI: the FxRackBank methods and the seven plate setters.  Without a GPU construction throws
 * OLFX_E_NODEVICE (exit 2); with one the setters land in their OLFX_PR_* fields, a control change
 * reaches the plate, and a block in each topology is audible where the kind says it is (exit 0).
 * Built and run by tests/test_platerack_host.py.
 */
#include <cstdio>
#include <vector>

#include "olfx_fx.hpp"

int main() {
    try {
        olfx::PlateRackBank bank(2, 48000.f);
        int bad = 0;
        auto expect = [&](bool ok, const char *what) { if (!ok) { std::printf("FAILED: %s\n", what); ++bad; } };
        bank.SetPredelay(1, 0.01f);
        bank.SetPrefilter(1, 0.6f);
        bank.SetInputDiffusion1(1, 0.61f);
        bank.SetInputDiffusion2(1, 0.62f);
        bank.SetDecayDiffusion(1, 0.63f);
        bank.SetDecay(1, 0.64f);
        bank.SetDamping(1, 0.65f);
        const float want[OLFX_DT_NPARAMS] = {0.01f, 0.6f, 0.61f, 0.62f, 0.63f, 0.64f, 0.65f};
        for (uint32_t f = 0; f < OLFX_DT_NPARAMS; ++f) expect(bank.get(1, OLFX_PR_VERB0 + f) == want[f], "plate setter field");
        expect(bank.get(0, OLFX_PR_VERB0 + OLFX_DT_DECAY) == 0.5f, "default decay");
        bank.SetTopology(1, olfx::FxRackBank::Topology::DaisyFirmware);
        bank.UpdateHardwareControl(0, 32, 0.7f);              /* CC_REVERB_TIME -> decay */
        expect(bank.get(0, OLFX_PR_VERB0 + OLFX_DT_DECAY) == 0.7f, "CC_REVERB_TIME");
        bank.set(0, OLFX_FR_DELAY_TIME, 0.001f);
        bank.set(1, OLFX_FR_DELAY_TIME, 0.001f);
        bank.set(1, OLFX_PR_VERB0 + OLFX_DT_PREDELAY, 0.f);
        const uint32_t F = 2048, n = 2;
        std::vector<float> x((size_t)2 * F * n), y((size_t)2 * F * n, 0.f);
        uint32_t s = 12345u;
        for (float &v : x) { s ^= s << 13; s ^= s >> 17; s ^= s << 5; v = (float)(int32_t)s * 2.3283064e-10f; }
        bank.Process(x.data(), y.data(), F);
        bool l0 = false, l1 = false, r0 = false, r1 = false;
        for (uint32_t f = 0; f < F; ++f) {
            l0 = l0 || y[(size_t)f * n] != 0.f;
            l1 = l1 || y[(size_t)f * n + 1] != 0.f;
            r0 = r0 || y[((size_t)F + f) * n] != 0.f;
            r1 = r1 || y[((size_t)F + f) * n + 1] != 0.f;
        }
        expect(l0 && l1, "channel 0 is audible");
        expect(!r0, "FxRack<2>: channel 1 is 0");
        expect(r1, "firmware topology: channel 1 carries the plate");
        expect(std::string(bank.kernel_name()) == "platerack_block_v1", "kernel name");
        std::printf("%d problems\n", bad);
        return bad ? 1 : 0;
    } catch (const olfx::Error &e) {
        std::printf("olfx::Error: %s\n", e.what());
        return e.code() == OLFX_E_NODEVICE ? 2 : 1;
    }
}
