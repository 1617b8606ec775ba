// normal_groups.hpp -- welding unrolled vertices for rptr_hip_set_normal_groups (include/rptr_hip.h "recomputed normals").
// Most hosts hold unrolled vertices and no index buffer. Corners whose rest positions are BITWISE equal and whose uploaded normal words
// are equal become one group: smooth vertices weld, hard edges (equal positions under different normals) stay hard. Groups are numbered
// by first occurrence; scenes.normal_groups (Python) gives the same array element for element.
#pragma once
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>

namespace rptr {

// positions: 3 floats per unrolled vertex; normal_words: one uint32 per vertex (the normal half of its qnrm_uv word)
inline std::vector<uint32_t> normal_groups(const float *positions, const uint32_t *normal_words, size_t num_vertices) {
    struct Key {
        uint32_t v[4];
        bool operator==(const Key &o) const { return std::memcmp(v, o.v, sizeof(v)) == 0; }
    };
    struct Hash {
        size_t operator()(const Key &k) const {
            uint64_t h = 0xcbf29ce484222325ull; // FNV-1a over the four words
            for (uint32_t w : k.v) h = (h ^ w) * 0x100000001b3ull;
            return (size_t)h;
        }
    };
    std::unordered_map<Key, uint32_t, Hash> id_of;
    id_of.reserve(num_vertices);
    std::vector<uint32_t> out(num_vertices);
    for (size_t i = 0; i < num_vertices; ++i) {
        Key k;
        std::memcpy(k.v, positions + 3 * i, 12); // the bits, not the values: -0.0f and 0.0f are different corners, a NaN equals itself
        k.v[3] = normal_words[i];
        out[i] = id_of.emplace(k, (uint32_t)id_of.size()).first->second;
    }
    return out;
}

} // namespace rptr
