// Holds the pure step plans of mpmc_amd/csrc/step_plan.h to restatements written from their descriptions (sets, std::stable_sort,
// the schedule of the deferred sweeps) -- not from the engine's code.  Built and run by tests/test_step_plan.py with
// -fsanitize=address,undefined; exit status 0 = every check held.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "step_plan.h"

using namespace mpmc;

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            ++failures;                                   \
            fprintf(stderr, "FAILED %s: ", #cond);        \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, "\n");                        \
            if (failures > 20) exit(1);                   \
        }                                                 \
    } while (0)

static std::set<int> as_set(const BlockList &l) {
    std::set<int> s(l.blk, l.blk + l.n);
    if ((int)s.size() != l.n) ++failures, fprintf(stderr, "FAILED: a block listed twice\n");
    return s;
}

// ---- chain build plan
static void check_chain(bool fresh, int tail, int nt, int nlag, const std::vector<int> &slots) {
    std::set<int> changed;
    for (int s : slots) changed.insert(s / 64);
    if (tail >= 0)
        for (int b = tail; b < nt; ++b) changed.insert(b);
    const bool want_full = (int)changed.size() > kMaxBlockList || !fresh;
    GsBuild gb;
    const bool full = plan_chain_build(fresh, tail, nt, nlag, slots.data(), (int)slots.size(), gb);
    CHECK(full == want_full, "fresh %d tail %d nt %d nlag %d, %zu changed blocks", fresh, tail, nt, nlag, changed.size());
    CHECK(gb.Minv == nullptr && gb.nlag == 0, "the plan fills in the lists only");
    if (want_full) {
        CHECK(gb.nb_all == nt && gb.inv.n == 0 && gb.own.n == 0, "full: nb_all %d of %d, lists %d %d", gb.nb_all, nt, gb.inv.n, gb.own.n);
        for (int k = 0; k < kGsMaxLag; ++k) CHECK(gb.nb[k].n == 0, "full: lag list %d has %d entries", k + 1, gb.nb[k].n);
        return;
    }
    CHECK(gb.nb_all == 0, "nb_all %d", gb.nb_all);
    std::set<int> own(changed);
    own.erase(0);
    CHECK(as_set(gb.inv) == changed, "inv, nt %d tail %d", nt, tail);
    CHECK(as_set(gb.own) == own, "own, nt %d tail %d", nt, tail);
    for (int k = 1; k <= kGsMaxLag; ++k) {
        std::set<int> want;
        if (k <= nlag)
            for (int b : changed)
                if (b + k < nt && !own.count(b + k)) want.insert(b + k);
        CHECK(as_set(gb.nb[k - 1]) == want, "lag %d of %d, nt %d tail %d", k, nlag, nt, tail);
    }
}

static void chain_plans() {
    for (int nlag = 2; nlag <= 4; ++nlag) {
        for (int nt : {1, 2, 3, 5})
            for (unsigned mask = 0; mask < (1u << nt); ++mask) {  // every subset of blocks
                std::vector<int> slots;
                for (int b = nt - 1; b >= 0; --b)
                    if (mask >> b & 1u) slots.push_back(64 * b + (7 * b + 3) % 64);
                check_chain(true, -1, nt, nlag, slots);
                check_chain(false, -1, nt, nlag, slots);
                check_chain(true, nt - 1, nt, nlag, slots);  // the last block re-ordered as well
            }
        for (int nblocks : {48, 49}) {  // as many as a list holds, and one more
            std::vector<int> slots;
            for (int b = 0; b < nblocks; ++b) slots.push_back(64 * ((b * 7) % 60) + b);  // (7 and 60 coprime: distinct blocks)
            check_chain(true, -1, 60, nlag, slots);
        }
        check_chain(true, -1, 5, nlag, {64 * 2 + 1, 64 * 2 + 63});  // two slots of one block
        check_chain(true, -1, 5, nlag, {64 * 4 + 5, 64 * 4 + 5});   // the same slot twice, in the last block
        check_chain(true, 0, 5, nlag, {64 * 3 + 9});                // the whole view re-ordered, and a dirty slot in it
        check_chain(true, 3, 5, nlag, {64 * 1 + 9});                // a dirty slot in front of the re-ordered tail
        check_chain(true, 59, 60, nlag, {0, 64 * 30});
        check_chain(true, 12, 60, nlag, {64 * 3});                  // a tail of 48 blocks and one more in front: 49
    }
}

// ---- the chain kernel's grid: block t has main(t) and aux(t, k), k = 2 .. min(t, nlag) (kernels_gs_chain.h, "Work
// decomposition"), so max(1, min(t, nlag)) tickets, and gs_chain_ticket_base(t, nlag) counts those of the blocks in front of
// t -- the host's grid size with t = nt, and the kernel's own origin of block t's tickets.  (The kernel's decode of a ticket
// into a block and a lag is written out in gs_chain_kernel and is not reachable from here.)
static void chain_tickets() {
    for (int nlag = 2; nlag <= kGsMaxLag; ++nlag) {
        CHECK(gs_chain_ticket_base(0, nlag) == 0, "nlag %d: block 0 starts at ticket %d", nlag, gs_chain_ticket_base(0, nlag));
        int roles = 0;
        for (int t = 0; t < 300; ++t) {  // (nt = t + 1 = 1 .. 300)
            const int cnt = std::max(1, std::min(t, nlag));
            CHECK(gs_chain_ticket_base(t + 1, nlag) - gs_chain_ticket_base(t, nlag) == cnt, "nlag %d block %d", nlag, t);
            roles += cnt;
            CHECK(gs_chain_ticket_base(t + 1, nlag) == roles, "nlag %d nt %d: grid %d, roles %d", nlag, t + 1,
                  gs_chain_ticket_base(t + 1, nlag), roles);
        }
    }
}

// ---- ranked walk
static void check_walk(const std::vector<double> &metric, const std::vector<int> &order) {
    std::vector<int> want(order);
    std::stable_sort(want.begin(), want.end(), [&](int x, int y) { return metric[x] > metric[y]; });
    std::vector<int> got(order.size() + 1, -7);
    ranked_walk(metric.data(), order, got.data());
    CHECK(got.back() == -7, "wrote past nv = %zu", order.size());
    got.pop_back();
    CHECK(got == want, "nv %zu, first metric %g", order.size(), metric.empty() ? 0.0 : metric[0]);
}

static void ranked_walks() {
    for (int nv : {0, 1, 2, 64, 65}) {
        const int n = 2 * nv + 3;  // atoms; view 0 holds every other one, not in index order
        std::vector<int> order;
        for (int k = 0; k < nv; ++k) order.push_back(2 * k + 1);
        if (nv > 1) std::swap(order[0], order[nv - 1]);
        std::vector<double> m(n, 0.0);
        auto fill = [&](auto f) {
            for (int i = 0; i < n; ++i) m[i] = f(i);
        };
        fill([](int) { return 5.0; });  // all equal
        check_walk(m, order);
        fill([](int i) { return (double)i; });  // strictly increasing
        check_walk(m, order);
        fill([](int i) { return (double)(i % 3); });  // ties
        check_walk(m, order);
        fill([](int i) { return (double)((i * 7) % 4) * 341.0; });  // 0, 341, 682, 1023: the last value of the counting path
        check_walk(m, order);
        fill([](int i) { return i % 5 == 0 ? 1023.0 : (double)(i % 2); });
        check_walk(m, order);
        fill([](int i) { return i % 5 == 1 ? 1024.0 : (double)(i % 3); });  // the first value of the fallback
        check_walk(m, order);
        fill([](int i) { return i % 4 == 1 ? 2.5 : (double)(i % 3); });  // not a count
        check_walk(m, order);
        fill([](int i) { return i % 4 == 3 ? -1.0 : (double)(i % 3); });  // negative
        check_walk(m, order);
    }
}

// ---- deferred-sweep schedule
static void sweep_schedule() {
    for (int n = 1; n <= 8; ++n) {
        const int m = (n + 1) / 2;
        const bool odd = n % 2 == 1;
        for (int it = 1; it <= n; ++it) {
            const SweepParams sp = jacobi_sweep_params(it, n, 0.0, false, true, 1.0, 0.0);
            CHECK(((sp.energy_mode & kEnergyMid) != 0) == (it == m), "n %d sweep %d", n, it);
            CHECK(((sp.energy_mode & kEnergyPrevSums) != 0) == (it == m && odd), "n %d sweep %d", n, it);
            CHECK(((sp.energy_mode & kEnergyStoreSums) != 0) == (odd && n - m >= 1 && it == n - m), "n %d sweep %d", n, it);
            CHECK((sp.energy_mode & ~(kEnergyMid | kEnergyPrevSums | kEnergyStoreSums)) == 0, "n %d sweep %d", n, it);
            CHECK(sp.skip_sums == 1, "n %d sweep %d", n, it);
            CHECK(sp.err_slot == it && sp.want_err == 0 && sp.want_rrms == 0 && sp.w_new == 1.0 && sp.w_old == 0.0, "n %d sweep %d", n, it);
            for (int published = 0; published < 2; ++published)
                CHECK(sweep_is_pending(it, n, true, published) == (it == n || (published && it > m && it < n)),
                      "n %d sweep %d published %d", n, it, published);
            // without the deferral: the sums are skipped before sweep n and wanted at it; nothing is ever pending
            const SweepParams plain = jacobi_sweep_params(it, n, 0.0, true, false, 0.75, 0.25);
            CHECK(plain.skip_sums == (it < n ? 1 : 0) && plain.energy_mode == 0, "n %d sweep %d", n, it);
            CHECK(plain.want_rrms == 1 && plain.w_new == 0.75 && plain.w_old == 0.25, "n %d sweep %d", n, it);
            CHECK(!sweep_is_pending(it, n, false, false) && !sweep_is_pending(it, n, false, true), "n %d sweep %d", n, it);
        }
    }
    // precision-controlled: every sweep may be the last, the host reads the error after each
    const SweepParams p = jacobi_sweep_params(3, 10, 1e-4, true, false, 1.0, 0.0);
    CHECK(p.skip_sums == 0 && p.want_err == 1 && p.err_slot == 3, "precision mode");
    double w_new, w_old;
    mixing_weights(false, false, 1.03, 4, w_new, w_old);
    CHECK(w_new == 1.0 && w_old == 0.0, "plain");
    mixing_weights(true, false, 1.03, 4, w_new, w_old);
    CHECK(w_new == 1.03 && w_old == 1.0 - 1.03, "sor");
    mixing_weights(false, true, 0.5, 4, w_new, w_old);
    CHECK(w_old == std::exp(-2.0) && w_new == 1.0 - w_old, "esor");
}

// ---- blocks_of, chunking, placement
static void small_plans() {
    DirtyBlocks d;
    CHECK(blocks_of({0, 63}, d) && d.n == 1 && d.blk[0] == 0, "one block");
    CHECK(blocks_of({63, 64}, d) && d.n == 2 && d.blk[0] == 0 && d.blk[1] == 1, "two blocks");
    CHECK(blocks_of({130, 5, 129, 5, 190}, d) && d.n == 2 && d.blk[0] == 2 && d.blk[1] == 0, "duplicates count once");
    CHECK(blocks_of({}, d) && d.n == 0, "no atom");
    std::vector<int> atoms;
    for (int b = 0; b < 16; ++b) atoms.push_back(64 * (3 * b) + b);
    CHECK(blocks_of(atoms, d) && d.n == 16, "16 distinct blocks fit");
    for (int b = 0; b < 16; ++b) CHECK(d.blk[b] == 3 * b, "block %d", b);
    atoms.push_back(64 * 100);
    CHECK(!blocks_of(atoms, d), "17 do not");
    CHECK(d.n == 0, "... and leave a zeroed list");
    for (int b = 0; b < kMaxDirtyBlocks; ++b) CHECK(d.blk[b] == 0, "zeroed entry %d", b);

    // chunks of whole tiles that cover npad, no more of them than tiles, about target / ntile of them
    for (int npad = 128; npad <= 128 * 200; npad += 128)
        for (int target : {2048, 4096}) {
            const ChunkPlan cp = chunk_plan(npad, target);
            const int ntile = npad / 64;
            CHECK(cp.chunk % 64 == 0 && cp.nchunk >= 1 && cp.nchunk <= ntile, "npad %d", npad);
            CHECK((long)cp.nchunk * cp.chunk >= npad && (long)(cp.nchunk - 1) * cp.chunk < npad, "npad %d", npad);
            CHECK(cp.nchunk <= std::max(1, target / ntile), "npad %d", npad);
        }

    int first, hole;
    const std::vector<std::pair<int, int>> holes = {{10, 3}, {40, 5}, {20, 3}};
    CHECK(place_molecule(holes, 100, 120, 3, first, hole) && first == 20 && hole == 2, "the most recent hole of that size");
    CHECK(place_molecule(holes, 100, 120, 5, first, hole) && first == 40 && hole == 1, "hole of 5");
    CHECK(place_molecule(holes, 100, 120, 4, first, hole) && first == 100 && hole == -1, "no such hole: at the end");
    CHECK(place_molecule(holes, 100, 104, 4, first, hole) && first == 100, "just fits");
    CHECK(!place_molecule(holes, 100, 103, 4, first, hole), "full");
    const std::vector<int> slot_of_atom = {0, -1, 1, -1};
    const double pol[3] = {1.0, 0.0, 2.0};
    CHECK(count_new_view_slots(slot_of_atom, false, 0, 3, pol) == 0, "both sites take their atoms' old view slots");
    CHECK(count_new_view_slots(slot_of_atom, false, 1, 3, pol) == 2, "neither has one");
    CHECK(count_new_view_slots(slot_of_atom, true, 0, 3, pol) == 2, "Gauss-Seidel modes: always new");
    CHECK(count_new_view_slots(slot_of_atom, false, 3, 3, pol) == 2, "past the end of the map");
}

int main() {
    chain_plans();
    chain_tickets();
    ranked_walks();
    sweep_schedule();
    small_plans();
    if (failures) fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
