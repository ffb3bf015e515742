// tests/golden/rms_recorder.cpp -- records what the reference's own ol::core::Rms returns, for
// tests/golden/rms_reference_runs.json (gen_rms_golden.py) and for tests/test_meter_ref.py, which records
// again wherever the reference tree is present.  It includes the reference's header by path (-I
// <reference>/modules) and holds none of its text; it is built into a temporary directory, never into the tree.
//
//   rms_recorder <sample_rate> <window> [<frame> <sample_rate> <window>]  < x.f32  > rms.f32
//
// Init(sample_rate, window), then Process over the raw float32 samples on stdin, each result written as raw
// float32; the optional triple is a second Init just before that frame.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "corelib/ol_corelib.h"

int main(int argc, char **argv) {
    if (argc != 3 && argc != 6) return 2;
    ol::core::Rms rms;
    rms.Init((t_sample)std::atof(argv[1]), (t_sample)std::atof(argv[2]));
    const long again = argc == 6 ? std::atol(argv[3]) : -1;
    std::vector<float> x(4096), y(4096);
    long frame = 0;
    for (size_t got; (got = std::fread(x.data(), 4, x.size(), stdin)) > 0;) {
        for (size_t k = 0; k < got; ++k, ++frame) {
            if (frame == again) rms.Init((t_sample)std::atof(argv[4]), (t_sample)std::atof(argv[5]));
            y[k] = rms.Process(x[k]);
        }
        if (std::fwrite(y.data(), 4, got, stdout) != got) return 1;
    }
    return 0;
}
