// Driver of tests/test_batch_plan_host.py: the host rules of the batch sketcher (finch_rs_amd/csrc/fh_batch_plan.h) on their own,
// without HIP.  It computes nothing itself: every line of standard input is a question -- a function of the header and its
// arguments as numbers -- and the answer goes to standard output, one line each; the test asks and checks with arithmetic of
// its own.  A form is 0 small, 1 wide, 2 large, 3 counts.
//   check  form kind k size scale mask max_files stage         -> code message
//   geom   form kind k size max_files stage                    -> cap live_cap shard_cap rows out_stride out_words header data dev
//   tau    form kind size max_hash len large_want              -> tau
//   taken  kind size sorted overflow need_big n_coll n_live sp_count inserted_total tau -> 0 | 1
//   match  (form device max_files data_bytes k size seed kind scale) x 2: parked, asked -> 0 | 1
//   plan   kind k kmers_to_sketch final_size scale filter_on n_files -> ok form group_n
//   fit    st_size max_hash                                    -> 0 | 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fh_batch_plan.h"

namespace bp = fh::bplan;

struct Args {
    std::vector<std::string> v;
    size_t at = 1;
    const std::string &next() {
        if (at >= v.size()) {
            fprintf(stderr, "too few arguments: %s\n", v.empty() ? "" : v[0].c_str());
            exit(2);
        }
        return v[at++];
    }
    uint64_t u() { return strtoull(next().c_str(), nullptr, 0); }
    double d() { return strtod(next().c_str(), nullptr); }
    bp::Form form() { return (bp::Form)u(); }
    bp::PoolKey key() {
        bp::PoolKey k{};
        k.form = form();
        k.device = (int)u();
        k.max_files = (uint32_t)u();
        k.data_bytes = u();
        k.p.k = (uint32_t)u();
        k.p.size = u();
        k.p.seed = u();
        k.p.kind = (uint32_t)u();
        k.p.scale = d();
        return k;
    }
};

int main() {
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        Args a;
        for (char *t = strtok(line, " \n"); t; t = strtok(nullptr, " \n")) a.v.push_back(t);
        if (a.v.empty()) continue;
        const std::string &cmd = a.v[0];
        if (cmd == "check") {
            const bp::Form form = a.form();
            fh_params p{};
            p.kind = (uint32_t)a.u();
            p.k = (uint32_t)a.u();
            p.size = a.u();
            p.scale = a.d();
            p.hash_mask = a.u();
            const uint32_t max_files = (uint32_t)a.u();
            const bp::Verdict v = bp::check(form, &p, max_files, a.u());
            printf("%d %s\n", v.code, v.msg);
        } else if (cmd == "geom") {
            const bp::Form form = a.form();
            fh_params p{};
            p.kind = (uint32_t)a.u();
            p.k = (uint32_t)a.u();
            p.size = a.u();
            const uint32_t max_files = (uint32_t)a.u();
            const bp::Geometry g = bp::geometry(form, p, max_files, a.u());
            printf("%u %u %u %llu %u %llu %llu %llu %llu\n", g.cap, g.live_cap, g.shard_cap, (unsigned long long)g.rows, g.out_stride, (unsigned long long)g.out_words,
                   (unsigned long long)g.header_bytes, (unsigned long long)g.data_bytes, (unsigned long long)g.dev_bytes);
        } else if (cmd == "tau") {
            const bp::Form form = a.form();
            const uint32_t kind = (uint32_t)a.u();
            const uint64_t size = a.u(), max_hash = a.u(), len = a.u();
            printf("%llu\n", (unsigned long long)bp::tau(form, kind, size, max_hash, len, a.u()));
        } else if (cmd == "taken") {
            const uint32_t kind = (uint32_t)a.u();
            const uint64_t size = a.u();
            bp::Outcome c{};
            c.sorted = (uint32_t)a.u();
            c.overflow = (uint32_t)a.u();
            c.need_big = (uint32_t)a.u();
            c.n_coll = (uint32_t)a.u();
            c.n_live = (uint32_t)a.u();
            c.sp_count = a.u();
            c.inserted_total = a.u();
            printf("%d\n", bp::taken(kind, size, c, a.u()) ? 1 : 0);
        } else if (cmd == "match") {
            const bp::PoolKey parked = a.key();
            printf("%d\n", bp::pool_match(parked, a.key()) ? 1 : 0);
        } else if (cmd == "plan") {
            const uint32_t kind = (uint32_t)a.u(), k = (uint32_t)a.u();
            const uint64_t kmers = a.u(), final_size = a.u();
            const double scale = a.d();
            const int filter_on = (int)strtol(a.next().c_str(), nullptr, 0);
            const bp::FilePlan f = bp::plan_files(kind, k, kmers, final_size, scale, filter_on, (uint32_t)a.u());
            printf("%d %d %llu\n", f.ok ? 1 : 0, (int)f.form, (unsigned long long)f.group_n);
        } else if (cmd == "fit") {
            const uint64_t st_size = a.u();
            printf("%d\n", bp::scaled_may_fit(st_size, a.u()) ? 1 : 0);
        } else {
            fprintf(stderr, "unknown question: %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
