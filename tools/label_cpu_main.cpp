// label_cpu_main.cpp -- the host labeller as a stand-alone program, for a run under the host
// sanitizers (no GPU, no Python).  Labels noisy all-zero-codeword rows of a (64,20) + CRC-6 code with
// pscl_label_cpu on 1 and on 3 threads, with one sent message and with one per frame, and checks the
// four results against each other and the counts against the entries.
//
//   hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Ipolar_code_amd/csrc \
//       tools/label_cpu_main.cpp polar_code_amd/csrc/scl_cpu.cpp -o _out/label_cpu_main && _out/label_cpu_main
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "polar_scl.h"

int main() {
    const int N = 64, K = 20, L = 4, B = 96, T = 8;
    const uint64_t poly = 0x61;
    std::vector<int32_t> info;
    for (int i = 0; i < N && (int)info.size() < K; ++i)  // the phases of largest bit weight, ascending
        if (__builtin_popcount((unsigned)i) >= 4) info.push_back(i);
    for (int i = N - 1; (int)info.size() < K; --i)
        if (__builtin_popcount((unsigned)i) == 3) info.push_back(i);
    for (size_t a = 1; a < info.size(); ++a)
        for (size_t b = a; b > 0 && info[b - 1] > info[b]; --b) {
            const int32_t t = info[b];
            info[b] = info[b - 1];
            info[b - 1] = t;
        }
    std::vector<double> llr((size_t)B * N);
    uint64_t s = 0x9E3779B97F4A7C15ULL;
    for (size_t i = 0; i < llr.size(); ++i) {  // the all-zero codeword (+2) under coarse noise: ties among |L0|
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        llr[i] = 2.0 + ((double)(int)((s >> 40) % 17) - 8.0) * 0.5;
    }
    std::vector<int8_t> one((size_t)K, 0), per((size_t)B * K, 0);  // the zero message passes any CRC
    struct Out {
        std::vector<int64_t> frame;
        std::vector<float> a;
        std::vector<int32_t> flip, rank;
        int64_t counts[PSCL_NLABEL];
    };
    Out o[4];
    for (int v = 0; v < 4; ++v) {
        o[v].frame.assign((size_t)B, -1);
        o[v].a.assign((size_t)B * K, -1.0f);
        o[v].flip.assign((size_t)B, -9);
        o[v].rank.assign((size_t)B, -9);
        const int rc = pscl_label_cpu(N, info.data(), K, L, poly, llr.data(), B, (v & 1) ? per.data() : one.data(), (v & 1) ? K : 0,
                                      T, o[v].frame.data(), o[v].a.data(), o[v].flip.data(), (v & 2) ? nullptr : o[v].rank.data(),
                                      o[v].counts, (v & 2) ? 3 : 1);
        if (rc) return printf("pscl_label_cpu (variant %d): %d\n", v, rc), 1;
    }
    const int64_t A = o[0].counts[PSCL_LBL_ENTRIES];
    int64_t lab = 0;
    for (int64_t e = 0; e < A; ++e) lab += o[0].flip[(size_t)e] >= 0;
    if (A < 1 || lab != o[0].counts[PSCL_LBL_LABELLED] || A - lab != o[0].counts[PSCL_LBL_UNREPAIRED] ||
        o[0].counts[PSCL_LBL_DECODES] < A || o[0].counts[PSCL_LBL_DECODES] > A * T)
        return printf("counts do not add up\n"), 1;
    if (A < B && (o[0].frame[(size_t)A] != -1 || o[0].flip[(size_t)A] != -9)) return printf("rows past the entries written\n"), 1;
    for (int v = 1; v < 4; ++v)
        if (memcmp(o[v].counts, o[0].counts, sizeof(o[0].counts)) || o[v].frame != o[0].frame || o[v].flip != o[0].flip ||
            memcmp(o[v].a.data(), o[0].a.data(), sizeof(float) * (size_t)A * K) || (!(v & 2) && o[v].rank != o[0].rank))
            return printf("variant %d differs\n", v), 1;
    printf("ok: %lld entries, %lld labelled, %lld decodes\n", (long long)A, (long long)lab, (long long)o[0].counts[PSCL_LBL_DECODES]);
    return 0;
}
