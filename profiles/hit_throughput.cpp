// hit_throughput.cpp — cache-hit throughput of the C++ host mirror on one thread: bare IsConsistent() and
// ComputedRegistry::TryUseExisting on 256 Consistent nodes. It uses only members the mirror
// had before the state view, so the same source builds against a tree whose state read is fgi_get_state
// (a device round trip per read) and against one that reads the host-memory view:
//   g++ -O2 -std=c++17 -I<tree>/stl.fusion_amd/host profiles/hit_throughput.cpp \
//       -L<tree>/stl.fusion_amd/host/build -lfusion -L<tree>/stl.fusion_amd/lib -lfgi -o hit_throughput
// Each leg runs for about 1.5 s or 4 M reads, whichever comes first. Needs a GPU.
#include <chrono>
#include <cstdio>
#include <string>
#include <vector>

#include "fusion.hpp"

using namespace fusion;
using clk = std::chrono::steady_clock;

template <class F>
static double rate(F&& one) {
    const auto t0 = clk::now();
    uint64_t n = 0, hits = 0;
    double s = 0;
    do {
        for (int i = 0; i < 256; ++i) hits += one((int)(n + i) & 255) ? 1 : 0;
        n += 256;
        s = std::chrono::duration<double>(clk::now() - t0).count();
    } while (s < 1.5 && n < (4u << 20));
    if (hits != n) std::fprintf(stderr, "misses: %llu of %llu\n", (unsigned long long)(n - hits), (unsigned long long)n);
    return (double)n / s;
}

int main(int argc, char** argv) {
    const char* tag = argc > 1 ? argv[1] : "tree";
    ComputedRegistry r(1024);
    std::vector<std::shared_ptr<Computed>> nodes;
    std::vector<std::string> names;
    for (int i = 0; i < 256; ++i) {
        names.push_back("svc.Get(" + std::to_string(i) + ")");
        auto c = r.BeginCompute(names.back());
        r.SetOutput(*c);
        nodes.push_back(c);
    }
    const double a = rate([&](int i) { return nodes[i]->IsConsistent(); });
    const double b = rate([&](int i) { return (bool)r.TryUseExisting(names[i]); });
    std::printf("{\"tree\": \"%s\", \"is_consistent_per_s\": %.0f, \"try_use_existing_per_s\": %.0f}\n", tag, a, b);
    return 0;
}
