// records_plan_host.cpp -- the host rules of the record sketcher (finch_rs_amd/csrc/fh_records_plan.h) asked line by line on
// stdin, answered line by line on stdout; tests/test_records_plan_host.py works out what the answers must be.  Texts travel as
// hex digits ("-" is the empty text).
//
//   maxpos                                              -> MAX_POS GROUP_RECORDS GROUP_STAGE ROWS_BUDGET
//   header <hex>                                        -> name_len comment_off comment_len
//   split <hex>                                         -> n, then per record: text0 text1 hdr0 hdr1 seq0 seq_length positions
//   route <kind> <k> <positions> <lds_on>               -> 1 = LDS, 0 = one by one
//   rows <kind> <size> <k> <positions>...               -> row0 of every record, then the sum
//   region <positions>                                  -> bytes of the record's two-bit region
//   group_n <kind> <kmers_to_sketch> <final_size>       -> the size the handle is made for
//   geom <kind> <size> <max_records> <stage_bytes>      -> header_bytes data_bytes rows_cap
//   check <kind> <k> <size> <scale> <mask> <max_records> <stage_bytes> -> code, then the message
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "fh_records_plan.h"

namespace rp = fh::rplan;

static std::vector<uint8_t> unhex(const std::string &h) {
    std::vector<uint8_t> v;
    if (h == "-") return v;
    for (size_t i = 0; i + 1 < h.size(); i += 2) v.push_back((uint8_t)std::stoul(h.substr(i, 2), nullptr, 16));
    return v;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "maxpos") {
            printf("%u %u %llu %llu\n", rp::MAX_POS, rp::GROUP_RECORDS, (unsigned long long)rp::GROUP_STAGE, (unsigned long long)rp::ROWS_BUDGET);
        } else if (what == "header") {
            std::string h;
            in >> h;
            const std::vector<uint8_t> t = unhex(h);
            const rp::HeaderSplit s = rp::split_header(t.data(), t.size());
            printf("%zu %zu %zu\n", s.name_len, s.comment_off, s.comment_len);
        } else if (what == "split") {
            std::string h;
            in >> h;
            // (an exact-size heap copy: the sanitizer sees any read past the text)
            const std::vector<uint8_t> t0 = unhex(h);
            uint8_t *t = new uint8_t[t0.size() ? t0.size() : 1];
            for (size_t i = 0; i < t0.size(); ++i) t[i] = t0[i];
            std::vector<rp::Record> recs;
            rp::split_records(t, t0.size(), recs);
            printf("%zu", recs.size());
            for (const rp::Record &r : recs)
                printf(" %llu %llu %llu %llu %llu %llu %llu", (unsigned long long)r.text0, (unsigned long long)r.text1, (unsigned long long)r.hdr0, (unsigned long long)r.hdr1,
                       (unsigned long long)r.seq0, (unsigned long long)r.seq_length, (unsigned long long)r.positions);
            printf("\n");
            delete[] t;
        } else if (what == "route") {
            uint32_t kind, k, on;
            uint64_t pos;
            in >> kind >> k >> pos >> on;
            printf("%d\n", rp::route(kind, k, pos, on != 0) == rp::Route::Lds ? 1 : 0);
        } else if (what == "rows") {
            uint32_t kind, k;
            uint64_t size, p;
            in >> kind >> size >> k;
            std::vector<uint64_t> pos;
            while (in >> p) pos.push_back(p);
            std::vector<uint64_t> row0(pos.size() + 1);
            const uint64_t sum = rp::assign_rows(kind, size, k, pos.data(), (uint32_t)pos.size(), row0.data());
            for (size_t i = 0; i < pos.size(); ++i) printf("%llu ", (unsigned long long)row0[i]);
            printf("%llu\n", (unsigned long long)sum);
        } else if (what == "region") {
            uint64_t p;
            in >> p;
            printf("%llu\n", (unsigned long long)rp::region_bytes(p));
        } else if (what == "group_n") {
            uint32_t kind;
            uint64_t kts, fin;
            in >> kind >> kts >> fin;
            printf("%llu\n", (unsigned long long)rp::group_n(kind, kts, fin));
        } else if (what == "geom") {
            fh_params p{};
            uint32_t max_records;
            uint64_t stage;
            in >> p.kind >> p.size >> max_records >> stage;
            const rp::Geometry g = rp::geometry(p, max_records, stage);
            printf("%llu %llu %llu\n", (unsigned long long)g.header_bytes, (unsigned long long)g.data_bytes, (unsigned long long)g.rows_cap);
        } else if (what == "check") {
            fh_params p{};
            uint32_t max_records;
            uint64_t stage;
            std::string scale;
            in >> p.kind >> p.k >> p.size >> scale >> p.hash_mask >> max_records >> stage;
            p.scale = std::stod(scale);
            const rp::Verdict v = rp::check(&p, max_records, stage);
            printf("%d %s\n", v.code, v.msg);
        } else {
            fprintf(stderr, "unknown question: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
