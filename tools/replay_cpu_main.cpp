// replay_cpu_main.cpp -- the host decision-LLR replay as a stand-alone program, for a run under the
// host sanitizers (no GPU, no Python).  Decodes one N = 1024 frame with pscl_decode_cpu, replays
// every candidate with pscl_path_llrs_cpu and compares the bit patterns.
//
//   hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Ipolar_code_amd/csrc \
//       tools/replay_cpu_main.cpp polar_code_amd/csrc/scl_cpu.cpp -o _out/replay_cpu_main && _out/replay_cpu_main
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "polar_scl.h"

int main() {
    const int N = 1024, K = 512, L = 4;
    std::vector<int32_t> info;
    for (int i = 0; i < N && (int)info.size() < K; ++i)  // the K phases of largest bit weight, in order
        if (__builtin_popcount((unsigned)i) >= 5) info.push_back(i);
    for (int i = 0; (int)info.size() < K; ++i)
        if (__builtin_popcount((unsigned)i) == 4) info.push_back(i);
    std::vector<int32_t> sorted(info);
    for (size_t a = 1; a < sorted.size(); ++a)
        for (size_t b = a; b > 0 && sorted[b - 1] > sorted[b]; --b) {
            const int32_t t = sorted[b];
            sorted[b] = sorted[b - 1];
            sorted[b - 1] = t;
        }
    std::vector<double> llr((size_t)N);
    uint64_t s = 0x9E3779B97F4A7C15ULL;
    for (int i = 0; i < N; ++i) {  // a fixed pseudo-random row around +2 (zeros of both signs among it)
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        llr[(size_t)i] = (double)(int)((s >> 40) % 13) - 4.0;
        if (llr[(size_t)i] == 0.0 && (s & 1)) llr[(size_t)i] = -0.0;
    }
    std::vector<int32_t> np(1);
    std::vector<int8_t> cands((size_t)L * K);
    std::vector<double> il((size_t)L * K), out((size_t)L * K), rows((size_t)L * N);
    int rc = pscl_decode_cpu(N, sorted.data(), K, L, 0, llr.data(), 1, nullptr, np.data(), nullptr, nullptr, nullptr, nullptr,
                             cands.data(), il.data(), 1);
    if (rc) return printf("pscl_decode_cpu: %d\n", rc), 1;
    for (int p = 0; p < np[0]; ++p) memcpy(rows.data() + (size_t)p * N, llr.data(), sizeof(double) * (size_t)N);
    rc = pscl_path_llrs_cpu(N, sorted.data(), K, rows.data(), np[0], cands.data(), out.data(), 2);
    if (rc) return printf("pscl_path_llrs_cpu: %d\n", rc), 1;
    if (memcmp(out.data(), il.data(), sizeof(double) * (size_t)np[0] * K)) return printf("replay differs\n"), 1;
    printf("ok: %d candidates, %d decision LLRs each\n", np[0], K);
    return 0;
}
