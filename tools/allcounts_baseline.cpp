// One-core baseline for tools/allcounts_bench.py: counts.rs's AllCountsSketcher::process loop restated in plain C++
// (normalize(false) + bit_kmers(k, false) + saturating_add), then total_bases_and_kmers and to_vec's walk.  NOT the
// reference binary: a restatement of its loop, labelled as such wherever its numbers are quoted.
//
//     allcounts_baseline FILE K      (FILE: packed reads, one '\0' behind every read)  -> "<seconds> <num_valid_kmers>"
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const int k = atoi(argv[2]);
    FILE *f = fopen(argv[1], "rb");
    if (!f || k < 1 || k > 16) return 2;
    std::vector<uint8_t> buf;
    uint8_t tmp[1 << 16];
    size_t got;
    while ((got = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
    fclose(f);
    int8_t code[256];
    for (int i = 0; i < 256; ++i) code[i] = -1;
    code['A'] = code['a'] = 0, code['C'] = code['c'] = 1, code['G'] = code['g'] = 2, code['T'] = code['t'] = code['U'] = code['u'] = 3;
    const uint64_t mask = (k == 32) ? ~0ull : ((1ull << (2 * k)) - 1);
    std::vector<uint32_t> counts((size_t)1 << (2 * k), 0);
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t m = 0;
    int run = 0;
    for (uint8_t b : buf) { // (records are separated by '\0', which breaks windows like any non-base byte)
        const int c = code[b];
        if (c < 0) {
            run = 0;
            continue;
        }
        m = ((m << 2) | (uint64_t)c) & mask;
        if (++run >= k) {
            uint32_t &x = counts[m];
            x = x == UINT32_MAX ? x : x + 1; // saturating_add(1)
        }
    }
    uint64_t total = 0;
    for (uint32_t x : counts) total += x;
    // to_vec (counts.rs:43-64)
    std::vector<uint32_t> clone(counts);
    uint64_t rows = 0, sink = 0;
    for (uint64_t ix = 0; ix < counts.size(); ++ix) {
        uint32_t count = clone[ix];
        if (!count) continue;
        uint64_t x = ~ix & mask, rc = 0;
        for (int i = 0; i < k; ++i) rc = (rc << 2) | (x & 3), x >>= 2;
        const uint32_t extra = counts[rc];
        clone[rc] = 0;
        count += extra;
        sink += count;
        ++rows;
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%.6f %llu\n", secs, (unsigned long long)total);
    fprintf(stderr, "rows %llu (%llu)\n", (unsigned long long)rows, (unsigned long long)sink);
    return 0;
}
