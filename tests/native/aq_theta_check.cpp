/* TEST INFRASTRUCTURE ONLY (tests/test_aq_edge.py compiles and runs it; no GPU).
 * csrc/aq_edge_dev.h -- the angle and the edge decision of the edge-based adaptive quantisation modes, written without a maths library so that host and device
 * compute the same bits -- against the reference's arithmetic over EVERY pair of Sobel gradients a picture of the given bit depth can produce
 * (|g| <= 16 x the largest sample: 8161^2 pairs at 8 bits, 32737^2 at 10).  The reference's arithmetic is restated here as its -O2 -ffast-math build performs it
 * (computeEdge, source/encoder/slicetype.cpp:140-152; the header's comment lists the steps), WITH the host maths library's double-precision atan2 -- that is the
 * function the reference calls.  tests/golden/aq_edge_golden.npz holds planes run through the reference's own computeEdge, which ties this restatement to the binary.
 *
 * usage: aq_theta_check <8|10>              prints "pairs N theta_diff A edge_diff B" and the first differing pairs; exit status 1 if any differ
 *        aq_theta_check <8|10> near <file>  writes the coprime pairs (int32 gv, gh) whose angle in degrees lies within one float ulp of an integer -- where a
 *                                           last-bit difference in any step would show -- for the device test
 * At most 16 threads. */
#include "aq_edge_dev.h"
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <thread>
#include <vector>

namespace {

struct RefOut { int theta, edge; float t, wrapped; };

inline RefOut reference(int gv, int gh, int white)
{
    const float gradientV = (float)gv, gradientH = (float)gh;
    const float radians = (float)atan2((double)gradientV, (double)gradientH);
    const float deg = radians * 180.0f;
    float theta = (float)((double)deg * (1.0 / 3.14159265));
    const float before = theta;
    if (theta < 0) theta = theta + 180.0f;
    const float threshold = (float)white;
    RefOut o;
    o.theta = white > 255 ? (int)(uint16_t)theta : (int)(uint8_t)theta;
    o.edge = gradientH * gradientH + gradientV * gradientV >= threshold * threshold ? white : 0;
    o.t = before; o.wrapped = theta;
    return o;
}

int gcd(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

struct Part { uint64_t pairs = 0, thetaDiff = 0, edgeDiff = 0; std::vector<int32_t> first, near; };

}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s <8|10> [near <file>]\n", argv[0]); return 2; }
    const int depth = atoi(argv[1]), white = (1 << depth) - 1, gmax = 16 * white;
    const bool near = argc >= 4 && !strcmp(argv[2], "near");
    const int nthr = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<Part> parts(nthr);
    std::vector<std::thread> threads;
    for (int t = 0; t < nthr; t++)
        threads.emplace_back([&, t]() {
            Part& p = parts[t];
            for (int gv = -gmax + t; gv <= gmax; gv += nthr)
                for (int gh = -gmax; gh <= gmax; gh++)
                {
                    const RefOut r = reference(gv, gh, white);
                    if (near)
                    {
                        if (gcd(abs(gv), abs(gh)) != 1) continue;
                        auto close = [](float v) { return floorf(nextafterf(v, -INFINITY)) != floorf(v) || floorf(nextafterf(v, INFINITY)) != floorf(v); };
                        if (close(r.t) || close(r.wrapped)) { p.near.push_back(gv); p.near.push_back(gh); }
                        continue;
                    }
                    const int theta = xa_edge_theta(gv, gh), edge = xa_edge_is_edge(gv, gh, white) ? white : 0;
                    p.pairs++;
                    if (theta != r.theta) p.thetaDiff++;
                    if (edge != r.edge) p.edgeDiff++;
                    if ((theta != r.theta || edge != r.edge) && p.first.size() < 6 * 8)
                    { const int32_t rec[6] = { gv, gh, theta, r.theta, edge, r.edge }; p.first.insert(p.first.end(), rec, rec + 6); }
                }
        });
    for (auto& th : threads) th.join();
    if (near)
    {
        std::vector<int32_t> all;
        for (const Part& p : parts) all.insert(all.end(), p.near.begin(), p.near.end());
        FILE* f = fopen(argv[3], "wb");
        if (!f || fwrite(all.data(), 4, all.size(), f) != all.size()) { perror(argv[3]); return 2; }
        fclose(f);
        printf("near %zu\n", all.size() / 2);
        return 0;
    }
    Part sum;
    for (const Part& p : parts) { sum.pairs += p.pairs; sum.thetaDiff += p.thetaDiff; sum.edgeDiff += p.edgeDiff; sum.first.insert(sum.first.end(), p.first.begin(), p.first.end()); }
    printf("pairs %llu theta_diff %llu edge_diff %llu\n", (unsigned long long)sum.pairs, (unsigned long long)sum.thetaDiff, (unsigned long long)sum.edgeDiff);
    for (size_t i = 0; i + 6 <= sum.first.size() && i < 6 * 32; i += 6)
        printf("gv %d gh %d: theta %d (reference %d) edge %d (reference %d)\n", sum.first[i], sum.first[i + 1], sum.first[i + 2], sum.first[i + 3], sum.first[i + 4], sum.first[i + 5]);
    return sum.thetaDiff || sum.edgeDiff ? 1 : 0;
}
