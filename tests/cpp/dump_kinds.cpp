// tests/cpp/dump_kinds.cpp -- everything the host core (ol_dsp_amd/csrc/olfx_host.cpp) says about a kind,
// as plain text for kind numbers 0..13 (0, 9 and 13 are kinds nobody has): the per-kind constants, the
// validation of every field, and the routing of every control.  tests/test_kind_table.py compares the
// output byte for byte with tests/golden/host_kinds.txt.  Only results that do not depend on libm are
// printed: bit patterns of exact values, codes, messages and field indices.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "../../ol_dsp_amd/csrc/olfx_host.h"

using namespace olfx;

namespace {

constexpr int kFirstKind = 0, kLastKind = 13;

std::string fmt(const char *f, ...) __attribute__((format(printf, 1, 2)));
std::string fmt(const char *f, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

// Lines keyed by an index (a field, a control); runs of consecutive indices with the same text print once.
struct Runs {
    std::vector<std::pair<int, std::string>> v;
    void add(int i, const std::string &s) { v.emplace_back(i, s); }
    void print(const char *what) const {
        for (size_t a = 0; a < v.size();) {
            size_t b = a;
            while (b + 1 < v.size() && v[b + 1].first == v[b].first + 1 && v[b + 1].second == v[a].second) ++b;
            if (a == b) std::printf("  %s %d: %s\n", what, v[a].first, v[a].second.c_str());
            else std::printf("  %s %d-%d: %s\n", what, v[a].first, v[b].first, v[a].second.c_str());
            a = b + 1;
        }
    }
};

uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// the topology field of the kinds that have a rack, else -1
int topology_field(int kind) {
    switch (kind) {
    case OLFX_KIND_FXRACK: return OLFX_FR_TOPOLOGY;
    case OLFX_KIND_PLATERACK: return OLFX_PR_RACK0 + OLFX_FR_TOPOLOGY;
    case OLFX_KIND_SYNTH:
    case OLFX_KIND_SYNTH_SVF: return OLFX_SY_RACK0 + OLFX_FR_TOPOLOGY;
    default: return -1;
    }
}

// a fresh two-instance shadow, its first block's records taken
void drain(host::Shadow &sh) {
    const host::PacketPlan pl = sh.plan(false);
    std::vector<uint32_t> buf(pl.words + 4);
    sh.fill_records(pl, buf.data());
}
void fresh(host::Shadow &sh, int kind) {
    sh.init(kind, 2, 48000.f);
    sh.reset();
    drain(sh);
}

std::string list_of(const std::vector<uint32_t> &v) {
    std::string s = "[";
    for (size_t k = 0; k < v.size(); ++k) s += fmt(k ? " %u" : "%u", v[k]);
    return s + "]";
}

void constants(int kind) {
    const uint32_t np = host::n_params_of(kind);
    std::printf("  n_params %u in %u out %u note_events %d voice %d synth %d voice_state_slots %u\n", np,
                host::in_channels(kind), host::out_channels(kind), (int)host::takes_note_events(kind),
                (int)is_voice_kind(kind), (int)is_synth_kind(kind), voice_state_slots(kind));
    float p[64] = {};
    host::default_params(kind, p);
    std::printf("  defaults");
    for (uint32_t f = 0; f < np; ++f) std::printf(" %08x", bits(p[f]));
    std::printf("\n");
    const host::Segments sg = host::coef_segments(kind);
    std::printf("  coef_segments %u: %u %u %u total %u\n", sg.nseg, sg.words[0], sg.words[1], sg.words[2], sg.total());
    for (const float sr : {44100.f, 48000.f, 96000.f}) {
        std::printf("  state_bytes sr %.0f:", sr);
        for (const uint32_t n : {1u, 63u, 64u, 65u}) std::printf(" %llu", (unsigned long long)host::state_bytes(kind, n, sr));
        std::printf("\n");
    }
    std::printf("  algorithmic_bytes_per_frame %.17g read %.17g\n", host::algorithmic_bytes_per_frame(kind),
                host::algorithmic_read_bytes_per_frame(kind));
    for (const uint32_t n : {1u, 65u}) {
        std::printf("  max_packet_words n %u: %zu", n, host::max_packet_words(kind, n));
        if (is_synth_kind(kind))
            for (const uint32_t voices : {1u, 4u, 8u})
                std::printf(" voices %u: %zu", voices, host::max_packet_words(kind, n, voices * ((n + 63u) & ~63u)));
        std::printf("\n");
    }
}

void validation(int kind) {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const std::pair<const char *, float> probes[] = {
        {"-1", -1.f}, {"-0", -0.f}, {"0", 0.f}, {"0.5", 0.5f}, {"1", 1.f}, {"2", 2.f}, {"3", 3.f}, {"4", 4.f},
        {"5", 5.f}, {"13.65", 13.65f}, {"13.66", 13.66f}, {"nan", nan}, {"inf", inf}};
    Runs runs;
    for (uint32_t f = 0; f < host::n_params_of(kind); ++f) {
        std::string line;
        for (const auto &pr : probes) {
            host::Shadow sh;
            fresh(sh, kind);
            sh.pre_changed = false;
            const int rc = sh.set_range(1, 1, f, 1, &pr.second);
            if (rc) line += fmt(" %s=%d'%s'", pr.first, rc, sh.msg);
            else line += fmt(" %s=ok:c%d%d,p%d,n%lld,d%s", pr.first, sh.configured[0], sh.configured[1], (int)sh.pre_changed,
                             (long long)sh.n_components, list_of(sh.dirty_list).c_str());
        }
        runs.add((int)f, line);
    }
    runs.print("set field");
}

// One control event on instance 1 of a fresh shadow at a topology (-1: the kind has no such field).
void routing(int kind, int topology) {
    const int tf = topology_field(kind);
    for (const int source : {(int)OLFX_CTL_MIDI, (int)OLFX_CTL_HARDWARE}) {
        Runs runs;
        for (int control = 0; control < 128; ++control) {
            host::Shadow sh;
            fresh(sh, kind);
            if (tf >= 0) {
                const float t[2] = {(float)topology, (float)topology};
                if (sh.set_range(0, 2, (uint32_t)tf, 1, t)) return;      // a topology this kind refuses
                drain(sh);
            }
            sh.pre_changed = false;
            // a value no control produces, so that a control that sets a field's default still shows
            const float mark = 1234.5f;
            for (uint32_t f = 0; f < sh.n_params; ++f)
                if ((int)f != tf) sh.params[(size_t)f * 2 + 1] = mark;
            const std::vector<float> before = sh.params;
            const olfx_control_event ev{1u, (uint8_t)control, (uint8_t)source, 0, source == OLFX_CTL_MIDI ? 64.f : 0.5f};
            const int rc = sh.control(&ev, 1);
            std::vector<uint32_t> changed;
            for (size_t k = 0; k < before.size(); ++k)
                if (bits(before[k]) != bits(sh.params[k])) changed.push_back((uint32_t)k);   // index = field * 2 + instance
            if (!rc && changed.empty() && !sh.configured[1] && sh.dirty_list.empty()) continue;
            std::string line = fmt("rc %d", rc);
            if (rc) line += fmt(" '%s'", sh.msg);
            line += " fields [";
            for (size_t k = 0; k < changed.size(); ++k) line += fmt(k ? " %u%s" : "%u%s", changed[k] / 2, changed[k] % 2 ? "" : "@0");
            line += fmt("] configured %d dirty %s", sh.configured[1], list_of(sh.dirty_list).c_str());
            runs.add(control, line);
        }
        std::printf("  topology %d source %d:\n", topology, source);
        runs.print("  control");
    }
}

std::string hits(int rc, const uint32_t *field) {
    std::string s = fmt("rc %d", rc);
    for (int h = 0; h < rc && h < 2; ++h) s += fmt(" %d", (int)field[h]);       // OLFX_FIELD_UPDATE_ONLY prints as -1
    return s;
}

void maps() {
    for (const int source : {(int)OLFX_CTL_MIDI, (int)OLFX_CTL_HARDWARE}) {
        const float value = source == OLFX_CTL_MIDI ? 64.f : 0.5f;
        for (int kind = kFirstKind; kind <= kLastKind; ++kind) {
            Runs runs;
            for (int control = 0; control < 128; ++control) {
                uint32_t field = 0;
                float v = 0.f;
                const int rc = olfx_control_map(kind, (uint8_t)control, source, value, &field, &v);
                runs.add(control, rc == OLFX_OK ? fmt("rc 0 %d", (int)field) : fmt("rc %d", rc));
            }
            std::printf("olfx_control_map kind %d source %d:\n", kind, source);
            runs.print("control");
        }
        {
            Runs runs;
            for (int control = 0; control < 128; ++control) {
                uint32_t field[2] = {0, 0};
                float v[2] = {0.f, 0.f};
                runs.add(control, hits(olfx_synth_control_map((uint8_t)control, source, value, field, v), field));
            }
            std::printf("olfx_synth_control_map source %d:\n", source);
            runs.print("control");
        }
        for (int kind = kFirstKind; kind <= kLastKind; ++kind)
            for (uint32_t topology = 0; topology <= 5; ++topology) {
                Runs runs;
                for (int control = 0; control < 128; ++control) {
                    uint32_t field[2] = {0, 0};
                    float v[2] = {0.f, 0.f};
                    runs.add(control, hits(olfx_synth_control_map_at(kind, topology, (uint8_t)control, source, value, field, v), field));
                }
                std::printf("olfx_synth_control_map_at kind %d topology %u source %d:\n", kind, topology, source);
                runs.print("control");
            }
    }
}

}  // namespace

int main() {
    for (int kind = kFirstKind; kind <= kLastKind; ++kind) {
        std::printf("kind %d\n", kind);
        constants(kind);
        validation(kind);
        if (topology_field(kind) < 0) routing(kind, -1);
        else for (int topology = 0; topology <= 5; ++topology) routing(kind, topology);
    }
    maps();
    return 0;
}
