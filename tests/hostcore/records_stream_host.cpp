// records_stream_host.cpp -- the host rules of the STREAMED record sketcher (finch_rs_amd/csrc/fh_records_plan.h: check_stream,
// stream_row_bound, stream_assign_rows, stream_geometry, route3) asked line by line on stdin, answered line by line on stdout;
// tests/test_records_stream_plan_host.py works out what the answers must be.
//
//   consts                                                                -> MAX_POS STREAM_CAP STREAM_MAX_POS STREAM_GROUP_RECORDS STREAM_GROUP_STAGE ROWS_BUDGET
//   route3 <kind> <k> <positions> <lds_on> <stream_on> <max_pos> <group_n> -> 0 = LDS, 1 = streamed, 2 = one by one
//   route <kind> <k> <positions> <lds_on>                                  -> 1 = LDS, 0 = one by one (the two-way rule, unchanged)
//   bound <kind> <size> <k> <positions>                                    -> the record's rows on a stream handle
//   rows <kind> <size> <k> <positions>...                                  -> row0 of every record, then the sum
//   geom <kind> <size> <max_records> <stage_bytes>                         -> header_bytes data_bytes rows_cap
//   check <kind> <k> <size> <scale> <mask> <max_records> <stage_bytes>     -> code, then the message
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "fh_records_plan.h"

namespace rp = fh::rplan;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "consts") {
            printf("%u %u %u %u %llu %llu\n", rp::MAX_POS, rp::STREAM_CAP, rp::STREAM_MAX_POS, rp::STREAM_GROUP_RECORDS, (unsigned long long)rp::STREAM_GROUP_STAGE,
                   (unsigned long long)rp::ROWS_BUDGET);
        } else if (what == "route3") {
            uint32_t kind, k, lds, st;
            uint64_t pos, max_pos, group_n;
            in >> kind >> k >> pos >> lds >> st >> max_pos >> group_n;
            const rp::Route3 r = rp::route3(kind, k, pos, lds != 0, st != 0, max_pos, group_n);
            printf("%d\n", r == rp::Route3::Lds ? 0 : r == rp::Route3::Stream ? 1 : 2);
        } else if (what == "route") {
            uint32_t kind, k, on;
            uint64_t pos;
            in >> kind >> k >> pos >> on;
            printf("%d\n", rp::route(kind, k, pos, on != 0) == rp::Route::Lds ? 1 : 0);
        } else if (what == "bound") {
            uint32_t kind, k;
            uint64_t size, pos;
            in >> kind >> size >> k >> pos;
            printf("%llu\n", (unsigned long long)rp::stream_row_bound(kind, size, k, pos));
        } else if (what == "rows") {
            uint32_t kind, k;
            uint64_t size, p;
            in >> kind >> size >> k;
            // (exact-size heap arrays: the sanitizer sees any access past them)
            std::vector<uint64_t> pos;
            while (in >> p) pos.push_back(p);
            uint64_t *row0 = new uint64_t[pos.size() ? pos.size() : 1];
            const uint64_t sum = rp::stream_assign_rows(kind, size, k, pos.data(), (uint32_t)pos.size(), row0);
            for (size_t i = 0; i < pos.size(); ++i) printf("%llu ", (unsigned long long)row0[i]);
            printf("%llu\n", (unsigned long long)sum);
            delete[] row0;
        } else if (what == "geom") {
            fh_params p{};
            uint32_t max_records;
            uint64_t stage;
            in >> p.kind >> p.size >> max_records >> stage;
            const rp::Geometry g = rp::stream_geometry(p, max_records, stage);
            printf("%llu %llu %llu\n", (unsigned long long)g.header_bytes, (unsigned long long)g.data_bytes, (unsigned long long)g.rows_cap);
        } else if (what == "check") {
            fh_params p{};
            uint32_t max_records;
            uint64_t stage;
            std::string scale;
            in >> p.kind >> p.k >> p.size >> scale >> p.hash_mask >> max_records >> stage;
            p.scale = std::stod(scale);
            const rp::Verdict v = rp::check_stream(&p, max_records, stage);
            printf("%d %s\n", v.code, v.msg);
        } else {
            fprintf(stderr, "unknown question: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
