// bvh4_encode_fuzz.cpp -- stand-alone fuzz of the node encoder (csrc/bvh4.h rp_bvh4_encode), built and run by
// tests/test_bvh_check_cpu.py: once plain, once with -fsanitize=address,undefined. Compile with -ffp-contract=off, like the library.
//
// Every node gets 1 to 4 children with adversarial float boxes. The program restates nothing of the encoder's arithmetic except the
// decoding the traversal uses -- plane = fl(origin + fl(q) * 2^(exp - 127)) -- and checks per child and axis:
//   containment  the lower plane is <= the child's lower bound, the upper plane >= its upper bound (zero tolerance);
//   origin       is the smallest lower bound of the children, bit for bit (or both zero);
//   exponent     is the smallest e in 1 .. 253 with 2^(e - 127) >= fl(extent / 254) (found by search, not by the bit trick);
//   tightness    bound - plane < 2 steps + one float spacing at the plane (tests/bvh_check.py derives it), where the extent and the
//                decoded plane are finite (beside FLT_MAX origin + q * step overflows to inf, which still contains);
//   empty slots  qlo = 255, qhi = 0; padding is zero.
// Exit status 0 and one summary line on success; 1 and the offending node on the first failure.
// usage: bvh4_encode_fuzz [nodes per case, default 40000] [seed]
#include "bvh4.h"

#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static float uni() { return (float)(rnd() >> 40) * (1.0f / 16777216.0f); } // [0, 1)
static float sym() { return 2.0f * uni() - 1.0f; }
static float pow2(int e) { return ldexpf(1.0f, e); }

// one coordinate interval [lo, hi] of a child, by case
static void interval(int kind, float &lo, float &hi) {
    float a = 0, b = 0;
    switch (kind) {
    case 0: // ordinary
        a = sym() * 10.0f;
        b = a + uni() * 5.0f;
        break;
    case 1: // a large offset with a tiny extent
        a = 1.0e6f + sym() * 0.1f;
        b = a + uni() * 0.1f;
        break;
    case 2: // sub-normal extents around zero
        a = (float)(int)(rnd() % 4096) * FLT_TRUE_MIN * (rnd() & 1 ? 1.0f : -1.0f);
        b = a + (float)(rnd() % 4096) * FLT_TRUE_MIN;
        break;
    case 3: // near FLT_MAX: the extent of the node overflows when the children lie on both sides
        a = (rnd() & 1 ? 1.0f : -1.0f) * 3.0e38f * (0.5f + 0.5f * uni());
        b = a + fabsf(a) * uni() * 0.1f;
        if (!(b <= FLT_MAX)) b = FLT_MAX;
        break;
    case 4: // a mix of binades 200 apart
        a = sym() * pow2((int)(rnd() % 200) - 100);
        b = a + uni() * pow2((int)(rnd() % 200) - 100);
        break;
    case 5: // signed zeros
        a = (rnd() & 1) ? -0.0f : 0.0f;
        b = (rnd() & 1) ? ((rnd() & 1) ? -0.0f : 0.0f) : uni() * pow2((int)(rnd() % 40) - 20);
        break;
    case 6: // lo == hi
        a = sym() * pow2((int)(rnd() % 80) - 40);
        b = a;
        break;
    default: // children that share planes with their siblings (grid aligned)
        a = (float)((int)(rnd() % 17) - 8) * 0.25f;
        b = a + (float)(rnd() % 5) * 0.25f;
        break;
    }
    if (b < a) {
        const float t = a;
        a = b;
        b = t;
    }
    lo = a;
    hi = b;
}

static bool same_bits_or_zero(float a, float b) { return rp_bits_of(a) == rp_bits_of(b) || (a == 0.0f && b == 0.0f); }
static float spacing(float x) {
    x = fabsf(x);
    if (!(x <= FLT_MAX)) return INFINITY;
    return nextafterf(x, INFINITY) - x;
}

static double g_worst = 0.0; // worst slack in steps

static int check(const RpBox4 &b, const int32_t child[4], int kind, long id) {
    RptrBvh4Node n;
    float nlo[3], nhi[3];
    rp_bvh4_encode(b, child, &n, nlo, nhi);
#define FAIL(...)                                                                            \
    do {                                                                                     \
        fprintf(stderr, "case %d node %ld: ", kind, id);                                     \
        fprintf(stderr, __VA_ARGS__);                                                        \
        fprintf(stderr, "\n");                                                               \
        return 1;                                                                            \
    } while (0)
    if (n._pad0 != 0 || n._pad1[0] != 0 || n._pad1[1] != 0) FAIL("padding is not zero");
    for (int a = 0; a < 3; ++a) {
        float lo = INFINITY, hi = -INFINITY;
        for (int k = 0; k < 4; ++k)
            if (child[k] != RPTR_BVH4_EMPTY) {
                if (b.lo[k][a] < lo) lo = b.lo[k][a];
                if (b.hi[k][a] > hi) hi = b.hi[k][a];
            }
        if (!same_bits_or_zero(n.origin[a], lo)) FAIL("axis %d origin %a, smallest lower bound %a", a, n.origin[a], lo);
        if (!same_bits_or_zero(nlo[a], lo) || !same_bits_or_zero(nhi[a], hi)) FAIL("axis %d node bounds [%a, %a], children [%a, %a]", a, nlo[a], nhi[a], lo, hi);
        const float extent = hi - lo, x = extent / 254.0f;
        int e = 1;
        while (e < 253 && !(pow2(e - 127) >= x)) ++e; // the smallest step that is >= extent / 254
        if (n.exp[a] != e) FAIL("axis %d exp %d, the smallest step >= %a / 254 has exp %d", a, n.exp[a], extent, e);
        const float step = pow2((int)n.exp[a] - 127);
        for (int k = 0; k < 4; ++k) {
            if (n.child[k] != child[k]) FAIL("slot %d child %d, given %d", k, n.child[k], child[k]);
            if (child[k] == RPTR_BVH4_EMPTY) {
                if (n.qlo[a][k] != 255 || n.qhi[a][k] != 0) FAIL("axis %d empty slot %d has the box %d, %d", a, k, n.qlo[a][k], n.qhi[a][k]);
                continue;
            }
            const float plo = n.origin[a] + (float)n.qlo[a][k] * step, phi = n.origin[a] + (float)n.qhi[a][k] * step;
            if (!(plo <= b.lo[k][a])) FAIL("axis %d slot %d: lower plane %a inside the child (%a)", a, k, plo, b.lo[k][a]);
            if (!(phi >= b.hi[k][a])) FAIL("axis %d slot %d: upper plane %a inside the child (%a)", a, k, phi, b.hi[k][a]);
            if (extent <= FLT_MAX && fabsf(plo) <= FLT_MAX && fabsf(phi) <= FLT_MAX) { // (near FLT_MAX the extent or origin + q * step overflows: still conservative)
                const double sl = (double)b.lo[k][a] - (double)plo, sh = (double)phi - (double)b.hi[k][a];
                if (!(sl < 2.0 * step + spacing(plo))) FAIL("axis %d slot %d: lower plane %.4f steps below the child", a, k, sl / step);
                if (!(sh < 2.0 * step + spacing(phi))) FAIL("axis %d slot %d: upper plane %.4f steps above the child", a, k, sh / step);
                if (sl / step > g_worst) g_worst = sl / step;
                if (sh / step > g_worst) g_worst = sh / step;
            }
        }
    }
#undef FAIL
    return 0;
}

int main(int argc, char **argv) {
    const long per_case = argc > 1 ? atol(argv[1]) : 40000;
    if (argc > 2) g_state ^= strtoull(argv[2], nullptr, 0);
    long nodes = 0;
    for (int kind = 0; kind < 9; ++kind) // 8: every axis of every child draws its own case
        for (long i = 0; i < per_case; ++i) {
            RpBox4 b;
            int32_t child[4];
            const int n_children = 1 + (int)(rnd() % 4);
            for (int k = 0; k < 4; ++k) {
                const bool used = k < n_children;
                child[k] = used ? ((rnd() & 1) ? (int32_t)(rnd() % 1000) : RPTR_BVH_LEAF(rnd() % 1000, 1 + rnd() % 4)) : RPTR_BVH4_EMPTY;
                for (int a = 0; a < 3; ++a) {
                    b.lo[k][a] = INFINITY;
                    b.hi[k][a] = -INFINITY;
                    if (used) interval(kind < 8 ? kind : (int)(rnd() % 8), b.lo[k][a], b.hi[k][a]);
                }
            }
            if (rnd() % 8 == 0 && n_children < 4) { // an empty slot in front of a used one
                const int k = (int)(rnd() % n_children);
                child[3] = child[k];
                child[k] = RPTR_BVH4_EMPTY;
                for (int a = 0; a < 3; ++a) {
                    b.lo[3][a] = b.lo[k][a];
                    b.hi[3][a] = b.hi[k][a];
                    b.lo[k][a] = INFINITY;
                    b.hi[k][a] = -INFINITY;
                }
            }
            if (check(b, child, kind, i)) return 1;
            ++nodes;
        }
    printf("bvh4 encoder fuzz: %ld nodes, worst slack %.6f steps\n", nodes, g_worst);
    return 0;
}
