// matrix_baseline.cpp -- minmer_matrix's loop (lib/src/distance.rs:345-364) restated in plain C++, one core: the host-side
// yardstick of tools/matrix_bench.py.  A restatement of the loop, not the reference binary.
//
//   matrix_baseline FILE        FILE: u64 R, u64 S, u64 ref[R], u64 off[S + 1], u64 hashes[off[S]], u32 counts[off[S]]
//   prints: seconds  matching-cells  checksum
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t R = 0, S = 0;
    if (fread(&R, 8, 1, f) != 1 || fread(&S, 8, 1, f) != 1 || R == 0) return 2;
    std::vector<uint64_t> ref(R), off(S + 1);
    if (fread(ref.data(), 8, R, f) != R || fread(off.data(), 8, S + 1, f) != S + 1) return 2;
    std::vector<uint64_t> hs(off[S]);
    std::vector<uint32_t> cs(off[S]);
    if (fread(hs.data(), 8, hs.size(), f) != hs.size() || fread(cs.data(), 4, cs.size(), f) != cs.size()) return 2;
    fclose(f);
    const auto t0 = std::chrono::steady_clock::now();
    int32_t *result = (int32_t *)calloc(S * R, sizeof(int32_t)); // Array2::zeros
    if (!result) return 3;
    uint64_t hits = 0;
    for (uint64_t i = 0; i < S; ++i) {
        uint64_t ref_pos = 0;
        for (uint64_t j = off[i]; j < off[i + 1]; ++j) {
            while (hs[j] > ref[ref_pos] && ref_pos < R - 1) ++ref_pos;
            if (hs[j] == ref[ref_pos]) {
                result[i * R + ref_pos] = (int32_t)cs[j];
                ++hits;
            }
        }
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    uint64_t sum = 0;
    for (uint64_t i = 0; i < S; ++i) sum += (uint32_t)result[i * R + (i * 2654435761u) % R]; // (keeps the loop's stores alive)
    printf("%.6f %llu %llu\n", secs, (unsigned long long)hits, (unsigned long long)sum);
    free(result);
    return 0;
}
