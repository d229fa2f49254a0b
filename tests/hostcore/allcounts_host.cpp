// Host build of the AllCounts window logic (finch_rs_amd/csrc/fh_counts.h) for tests/test_allcounts_model.py: the same
// ac_lane_windows the kernel runs, walked over a whole packed stream lane by lane (32 window starts per step, 48 bytes,
// bytes behind the end read as breakers), and ac_revcomp / ac_emit.
#include <cstring>

#include "../../finch_rs_amd/csrc/fh_counts.h"

using namespace fh;

template <int K>
static uint64_t windows_k(const uint8_t *seq, uint64_t len, uint32_t *out) {
    uint64_t n = 0;
    if (len < (uint64_t)K) return 0;
    const uint64_t n_pos = len - K + 1;
    for (uint64_t p = 0; p < n_pos; p += AC_LANE_POS) {
        uint8_t b[AC_LANE_BYTES] = {0};
        for (int i = 0; i < AC_LANE_BYTES; ++i)
            if (p + i < len) b[i] = seq[p + i];
        u32 d[12];
        memcpy(d, b, sizeof d);
        const uint64_t left = n_pos - p;
        ac_lane_windows<K>(d, left < 32 ? (u32)left : 32u, [&](int, u32 ix) { out[n++] = ix; });
    }
    return n;
}

// the index of every window, in stream order (out: room for len entries); -1 for k outside 1..16
extern "C" int64_t ac_host_windows(const uint8_t *seq, uint64_t len, int k, uint32_t *out) {
    switch (k) {
#define C(K) \
    case K: return (int64_t)windows_k<K>(seq, len, out);
        C(1) C(2) C(3) C(4) C(5) C(6) C(7) C(8) C(9) C(10) C(11) C(12) C(13) C(14) C(15) C(16)
#undef C
    default: return -1;
    }
}

extern "C" uint32_t ac_host_revcomp(uint32_t ix, int k) { return ac_revcomp(ix, k); }
extern "C" int ac_host_emit(uint32_t ix, uint32_t rc, uint32_t c, uint32_t crc) { return ac_emit(ix, rc, c, crc) ? 1 : 0; }
