// batch_driver.cpp -- host test of the many-call recorder (csrc/batch.hpp,
// csrc/batch.cpp; run by tests/test_batch_host.py, built by `make batch_asan`
// with ASan + UBSan on the host side).
//
// Op lists are built from tables of launch descriptions with a null stream and
// `one` / `merged` lambdas that only log, so no HIP call is ever made.  After
// flush() the log must show:
//   * every op issued exactly once, alone or as a member of exactly one group;
//   * each channel's ops in index order;
//   * every member of a group with the same non-null `many`, grid, block and
//     dynamic LDS, g.y == g.z == 1, and the same op index; groups of xcd ops
//     with g.x % 8 == 0;
//   * completeness: two ops of one index that could share a group do;
//   * merged_launches() == the number of groups of more than one op;
//   * nothing issued by a second flush();
//   * batch_active(): the recorder while recording, the previous recorder (or
//     null) during the issue and afterwards.
// Ops of kind 1 and 2 (event waits and records) need real events and are left
// to the GPU suite.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <tuple>
#include <vector>

#include "../../python-liquiddsp_amd/csrc/batch.hpp"

using ldsp::BatchOp;
using ldsp::BatchRecorder;

namespace {

int g_fail = 0;
const char* g_table = "";
#define CHECK(cond, ...)                                              \
    do {                                                              \
        if (!(cond)) {                                                \
            std::fprintf(stderr, "FAIL [%s] %s: ", g_table, #cond);   \
            std::fprintf(stderr, __VA_ARGS__);                        \
            std::fprintf(stderr, "\n");                               \
            if (++g_fail > 20) std::exit(1);                          \
        }                                                             \
    } while (0)

// The merged kernels of the tables: addresses only (never called).  xcd is a
// property of the kernel, as in the library (the modal IIR alone sets it).
const char kKernels[4] = {0, 0, 0, 0};
struct Kern {
    const void* many;
    bool xcd;
};
const Kern kNone{nullptr, false}, kA{&kKernels[0], false}, kB{&kKernels[1], false}, kX{&kKernels[2], true},
    kY{&kKernels[3], true};

struct Spec {
    Kern k;
    unsigned gx = 1, gy = 1, gz = 1, bx = 64;
    size_t shm = 0;
};
Spec S(Kern k, unsigned gx, unsigned bx = 64, size_t shm = 0, unsigned gy = 1, unsigned gz = 1)
{
    Spec s;
    s.k = k;
    s.gx = gx;
    s.gy = gy;
    s.gz = gz;
    s.bx = bx;
    s.shm = shm;
    return s;
}
using Table = std::vector<std::vector<Spec>>;     // [channel][op index]

struct Id {
    int c, i;
};
struct Issue {
    std::vector<Id> members;
    bool merged;
};

bool mergeable(const Spec& s) { return s.k.many && s.gy == 1 && s.gz == 1 && (!s.k.xcd || s.gx % 8 == 0); }
bool same_key(const Spec& a, const Spec& b)
{
    return a.k.many == b.k.many && a.gx == b.gx && a.gy == b.gy && a.gz == b.gz && a.bx == b.bx && a.shm == b.shm;
}

// Records `t` into a recorder nested in `outer` (may be null), flushes and checks.
void run_table(const char* name, const Table& t, BatchRecorder* outer)
{
    g_table = name;
    const int C = (int)t.size();
    std::vector<Issue> log;
    BatchRecorder* seen_during = reinterpret_cast<BatchRecorder*>(1);
    {
        BatchRecorder rec(C, nullptr);
        CHECK(ldsp::batch_active() == &rec, "not active while recording");
        CHECK(rec.stream() == nullptr, "stream");
        for (int c = 0; c < C; c++) {
            rec.channel(c);
            for (int i = 0; i < (int)t[c].size(); i++) {
                const Spec& s = t[c][i];
                BatchOp op;
                op.kind = 0;
                op.many = s.k.many;
                op.g = dim3(s.gx, s.gy, s.gz);
                op.b = dim3(s.bx, 1, 1);
                op.shm = s.shm;
                op.xcd = s.k.xcd;
                const Id id{c, i};
                op.args.resize(sizeof(Id));
                std::memcpy(op.args.data(), &id, sizeof(Id));
                op.one = [&log, &seen_during, id](hipStream_t) {
                    seen_during = ldsp::batch_active();
                    log.push_back(Issue{{id}, false});
                };
                if (s.k.many)
                    op.merged = [&log, &seen_during](hipStream_t, const std::vector<const BatchOp*>& grp) {
                        seen_during = ldsp::batch_active();
                        Issue is;
                        is.merged = true;
                        for (const BatchOp* o : grp) {
                            Id m;
                            std::memcpy(&m, o->args.data(), sizeof(Id));
                            is.members.push_back(m);
                        }
                        log.push_back(is);
                    };
                rec.add(std::move(op));
            }
            CHECK(ldsp::batch_active() == &rec, "not active while recording channel %d", c);
        }
        CHECK(log.empty(), "%zu ops issued before flush()", log.size());
        CHECK(rec.merged_launches() == 0, "merged_launches() before flush()");
        rec.flush();
        CHECK(ldsp::batch_active() == outer, "recorder still active after flush()");
        size_t total = 0;
        for (const auto& v : t) total += v.size();
        if (total) CHECK(seen_during == outer, "recorder active during the issue");

        // every op exactly once; per channel in index order
        std::map<std::pair<int, int>, int> count;
        std::vector<int> next((size_t)C, 0);
        int groups = 0;
        for (const Issue& is : log) {
            CHECK(!is.members.empty(), "empty issue");
            CHECK(is.merged == (is.members.size() > 1), "merged() for %zu ops", is.members.size());
            if (is.members.size() > 1) groups++;
            const Id f = is.members[0];
            std::set<int> chans;
            for (const Id& m : is.members) {
                CHECK(m.c >= 0 && m.c < C && m.i >= 0 && m.i < (int)t[m.c].size(), "op (%d, %d) out of range", m.c, m.i);
                if (m.c < 0 || m.c >= C || m.i < 0 || m.i >= (int)t[m.c].size()) return;
                count[{m.c, m.i}]++;
                CHECK(next[m.c] == m.i, "channel %d: op %d issued when %d was due", m.c, m.i, next[m.c]);
                next[m.c] = m.i + 1;
                CHECK(chans.insert(m.c).second, "channel %d twice in one group", m.c);
                if (is.members.size() > 1) {
                    const Spec &a = t[f.c][f.i], &b = t[m.c][m.i];
                    CHECK(m.i == f.i, "group mixes indices %d and %d", f.i, m.i);
                    CHECK(b.k.many != nullptr && same_key(a, b), "group of unequal launches (%d,%d) (%d,%d)", f.c, f.i,
                          m.c, m.i);
                    CHECK(b.gy == 1 && b.gz == 1, "group with g.y or g.z != 1");
                    CHECK(!b.k.xcd || b.gx % 8 == 0, "xcd group with g.x = %u", b.gx);
                }
            }
        }
        for (int c = 0; c < C; c++)
            for (int i = 0; i < (int)t[c].size(); i++)
                CHECK((count[{c, i}]) == 1, "op (%d, %d) issued %d times", c, i, (count[{c, i}]));
        CHECK(rec.merged_launches() == groups, "merged_launches() %d, groups %d", rec.merged_launches(), groups);

        // completeness: mergeable ops of one index with one key share a group
        std::map<std::pair<int, int>, int> where;
        for (size_t g = 0; g < log.size(); g++)
            for (const Id& m : log[g].members) where[{m.c, m.i}] = (int)g;
        for (int c = 0; c < C; c++)
            for (int c2 = c + 1; c2 < C; c2++)
                for (int i = 0; i < (int)std::min(t[c].size(), t[c2].size()); i++)
                    if (mergeable(t[c][i]) && mergeable(t[c2][i]) && same_key(t[c][i], t[c2][i]))
                        CHECK((where[{c, i}]) == (where[{c2, i}]), "ops (%d,%d) and (%d,%d) could merge and did not", c, i,
                              c2, i);

        const size_t issued = log.size();
        const int merged = rec.merged_launches();
        rec.flush();
        CHECK(log.size() == issued && rec.merged_launches() == merged, "a second flush() issued work");
        CHECK(ldsp::batch_active() == outer, "active recorder changed by a second flush()");
    }
    CHECK(ldsp::batch_active() == outer, "active recorder after the destructor");
}

void run_both(const char* name, const Table& t)
{
    run_table(name, t, nullptr);
    BatchRecorder outer(1, nullptr);              // a many-call inside a many-call (the nested case)
    run_table(name, t, &outer);
    g_table = name;
    CHECK(ldsp::batch_active() == &outer, "outer recorder not restored");
    outer.flush();
}

// A recorder destroyed without flush() (an exception between the objects)
// issues nothing and restores the previous recorder.
void run_abandoned()
{
    g_table = "abandoned";
    int issued = 0;
    {
        BatchRecorder rec(2, nullptr);
        BatchOp op;
        op.many = kA.many;
        op.g = dim3(4, 1, 1);
        op.b = dim3(64, 1, 1);
        op.one = [&issued](hipStream_t) { issued++; };
        rec.add(std::move(op));
    }
    CHECK(issued == 0 && ldsp::batch_active() == nullptr, "abandoned recorder");
}

Table repeat(int C, const std::vector<Spec>& list) { return Table((size_t)C, list); }

} // namespace

// the argument caps the suite's launch counts rest on
struct Arg432 {
    char b[432];
};
struct Arg64 {
    char b[64];
};
struct Arg3584 {
    char b[3584];
};
static_assert(ldsp::Many<Arg432>::kCap == 8, "modal IIR arguments: 8 objects per merged launch");
static_assert(ldsp::Many<Arg64>::kCap == 16, "small arguments: 16 objects per merged launch");
static_assert(ldsp::Many<Arg3584>::kCap == 1, "the largest arguments that still batch");
static_assert(sizeof(ldsp::Many<Arg432>) <= 4096 && sizeof(ldsp::Many<Arg64>) <= 4096, "kernarg limit");

int main()
{
    const std::vector<Spec> chain = {S(kA, 40, 256), S(kNone, 1, 64), S(kB, 40, 64, 4096), S(kX, 160, 256, 1024),
                                     S(kA, 1, 64)};
    // equal lists: everything merges
    for (int C : {1, 2, 8, 9, 16, 17}) run_both("equal", repeat(C, chain));
    {   // one list longer (a Costas modem among carrier ones: two more launches at the end)
        Table t = repeat(5, chain);
        t[2].push_back(S(kA, 7));
        t[2].push_back(S(kB, 7));
        run_both("longer", t);
    }
    {   // a shifted list: two extra launches in the middle move every later index
        Table t = repeat(6, chain);
        for (int c : {1, 4}) {
            t[c].insert(t[c].begin() + 1, S(kB, 3, 64));
            t[c].insert(t[c].begin() + 1, S(kA, 3, 64));
        }
        run_both("shifted", t);
    }
    {   // a different grid / block / shm / kernel / g.y / g.z in the middle
        Table t = repeat(7, chain);
        t[1][2] = S(kB, 41, 64, 4096);
        t[2][2] = S(kB, 40, 128, 4096);
        t[3][2] = S(kB, 40, 64, 0);
        t[4][2] = S(kA, 40, 64, 4096);
        t[5][2] = S(kB, 40, 64, 4096, 2);
        t[6][2] = S(kB, 40, 64, 4096, 1, 2);
        run_both("different", t);
    }
    {   // xcd launches: 147 never merges, 160 and 1024 do, each with its own
        Table t;
        for (unsigned gx : {147u, 160u, 1024u, 147u, 1024u, 160u, 147u, 1176u, 1176u})
            t.push_back({S(kA, 20), S(kX, gx, 256, 2048), S(kA, 20)});
        run_both("xcd", t);
        for (auto& v : t) v[1].k = kA;            // the same grids without xcd: every equal pair merges
        run_both("not xcd", t);
        for (auto& v : t) v[1].k = kY;
        t[0][1].k = kX;
        run_both("two xcd kernels", t);
    }
    {   // empty lists (n = 0 on some objects, or on all)
        Table t = repeat(4, chain);
        t[0].clear();
        t[2].clear();
        run_both("some empty", t);
        run_both("all empty", Table(3));
        run_both("one empty channel", Table(1));
    }
    {   // never-merged launches only
        run_both("no many", repeat(4, {S(kNone, 5), S(kNone, 5)}));
    }
    {   // the first object of an index cannot merge, later ones can
        Table t = {{S(kNone, 8)}, {S(kA, 8)}, {S(kA, 8, 64, 0, 2)}, {S(kA, 8)}, {S(kX, 147)}, {S(kX, 147)}, {S(kA, 8)}};
        run_both("late start", t);
    }
    run_abandoned();

    // seeded random tables: few distinct launches, so merges, partial groups and shifts abound
    std::mt19937 rng(20240607u);
    auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
    const Kern kerns[] = {kNone, kA, kA, kB, kX, kX, kY};
    const unsigned grids[] = {20, 147, 160, 1024, 1176};
    for (int it = 0; it < 4000; it++) {
        const int C = 1 + pick(it % 10 == 0 ? 17 : 6);
        std::vector<Spec> base;
        const int len = pick(7);
        for (int i = 0; i < len; i++)
            base.push_back(S(kerns[pick(7)], grids[pick(5)], pick(2) ? 64 : 256, pick(4) ? 0 : 4096));
        Table t;
        for (int c = 0; c < C; c++) {
            std::vector<Spec> v = base;
            const int edits = pick(3);
            for (int e = 0; e < edits; e++) {
                const int what = pick(5);
                const Spec s = S(kerns[pick(7)], grids[pick(5)], pick(2) ? 64 : 256, pick(4) ? 0 : 4096,
                                 pick(12) ? 1 : 2, pick(20) ? 1 : 2);
                if (what == 0 || v.empty()) v.insert(v.begin() + pick((int)v.size() + 1), s);
                else if (what == 1) v.erase(v.begin() + pick((int)v.size()));
                else if (what == 2) v.clear();
                else v[(size_t)pick((int)v.size())] = s;
            }
            t.push_back(v);
        }
        char name[32];
        std::snprintf(name, sizeof name, "random %d", it);
        if (it & 1) run_both(name, t);
        else run_table(name, t, nullptr);
    }

    g_table = "";
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
