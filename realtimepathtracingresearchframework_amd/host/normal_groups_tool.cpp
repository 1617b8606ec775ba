// normal_groups_tool.cpp -- host/normal_groups.hpp as a stand-alone program, for the tests (tests/test_normals_cpu.py builds it with sanitizers):
//   normal_groups_tool <in> <out>
// <in>: uint32 n, then n x 3 float32 rest positions, then n uint32 normal words (unrolled vertices); <out>: n uint32 group labels, what
// rptr_hip_set_normal_groups takes. Needs neither the library nor a device. Exit code 2 for a file that does not hold exactly that.
#include "normal_groups.hpp"

#include <cstdio>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: normal_groups_tool <in: uint32 n, n x 3 float32, n uint32> <out: n uint32>\n");
        return 2;
    }
    FILE *f = std::fopen(argv[1], "rb");
    uint32_t n = 0;
    bool ok = f && std::fread(&n, 4, 1, f) == 1;
    std::vector<float> positions(ok ? (size_t)n * 3 : 0);
    std::vector<uint32_t> words(ok ? (size_t)n : 0);
    if (ok && n) ok = std::fread(positions.data(), 4, positions.size(), f) == positions.size() && std::fread(words.data(), 4, words.size(), f) == words.size();
    ok = ok && std::fgetc(f) == EOF;
    if (f) std::fclose(f);
    if (!ok) {
        std::fprintf(stderr, "normal_groups_tool: %s does not hold uint32 n, n x 3 float32 and n uint32\n", argv[1]);
        return 2;
    }
    const std::vector<uint32_t> groups = rptr::normal_groups(positions.data(), words.data(), n);
    FILE *o = std::fopen(argv[2], "wb");
    ok = o && (groups.empty() || std::fwrite(groups.data(), 4, groups.size(), o) == groups.size());
    if (o) ok = std::fclose(o) == 0 && ok;
    if (!ok) {
        std::fprintf(stderr, "normal_groups_tool: cannot write %s\n", argv[2]);
        return 2;
    }
    return 0;
}
