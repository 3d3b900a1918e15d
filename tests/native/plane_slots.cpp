// The slot book of the solver's int8-limb workspace (csrc/gml_slots.h), driven on the host through the sequences the solver
// makes of it: first pass, trials, rejected trials, re-runs, scratch trials, a wrapped range, the restart from slot 0, and the
// FP64 path's convention.  usage: plane_slots R   (prints "ok" and exits 0, or the failed comparison and exits 1)
#include "gml_slots.h"

#include <cstdio>
#include <cstdlib>
#include <numeric>

using gml::PlaneSlots;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED line %d (R = %lld): %s\n", __LINE__, (long long)R, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

static int64_t R = 0;
static int64_t round32(int64_t a) { return (a + 31) / 32 * 32; }

static std::vector<int> range(int a, int b) {
    std::vector<int> v((size_t)(b - a));
    std::iota(v.begin(), v.end(), a);
    return v;
}

// what every state of the book must satisfy: a valid row owns the slot it points at, so no two valid rows share planes
static void check_book(const PlaneSlots &b) {
    std::vector<int> seen((size_t)b.capacity(), -1);
    for (int r = 0; r < (int)R; ++r) {
        CHECK(b.needs_refresh(r) == (b.stale(r) || b.slot(r) < 0));
        if (!b.valid(r)) continue;
        CHECK(b.slot(r) >= 0 && b.slot(r) < b.capacity() && b.owner_of(b.slot(r)) == r && !b.stale(r));
        CHECK(seen[b.slot(r)] < 0);
        seen[b.slot(r)] = r;
    }
    for (int64_t s = 0; s < b.capacity(); ++s) CHECK(b.owner_of(s) >= -1 && b.owner_of(s) < (int)R);
}

// a claim came out as a consecutive range at `base`, its padding owned by nobody
static void check_range(const PlaneSlots &b, const PlaneSlots::Range &g, const std::vector<int> &rows, int64_t base) {
    const int64_t n = (int64_t)rows.size();
    CHECK(g.lo == base && g.hi == base + round32(n) && g.lo % 32 == 0 && (int64_t)g.slot.size() == n);
    for (int64_t a = 0; a < n; ++a) CHECK(g.slot[a] == base + a && b.held({rows[a]}).slot[0] == base + a);
    for (int64_t s = base + n; s < g.hi; ++s) CHECK(b.owner_of(s) == -1);
}

struct Snapshot {
    std::vector<int> slot, owner;
    std::vector<bool> stale;
    explicit Snapshot(const PlaneSlots &b) {
        for (int r = 0; r < (int)R; ++r) slot.push_back(b.slot(r)), stale.push_back(b.stale(r));
        for (int64_t s = 0; s < b.capacity(); ++s) owner.push_back(b.owner_of(s));
    }
    bool operator==(const Snapshot &o) const { return slot == o.slot && owner == o.owner && stale == o.stale; }
};

static void int8_sequences(bool arm_half) {
    const int64_t Rp = round32(R);
    // the solver's formula for the int8 paths (Solver::init): both arms of the max occur over the sizes this program is run with
    const int64_t Smain = Rp + round32(std::max<int64_t>(R / 2, 96)) + 64, Scap = Smain + Rp;
    CHECK((R / 2 > 96) == arm_half);
    PlaneSlots b;
    CHECK(!b.reset(R, Rp - 32, Scap)); // a main range that a pass over every row would not fit: refused
    CHECK(!b.reset(R, Smain, Smain + Rp - 32));
    CHECK(b.reset(R, Smain, Scap));
    CHECK(b.capacity() == Scap);
    const std::vector<int> all = range(0, (int)R);
    for (int r : all) CHECK(b.needs_refresh(r) && !b.valid(r) && b.slot(r) == -1);
    check_book(b);

    // the first pass of a solve: every row, from slot 0
    PlaneSlots::Range g = b.claim(all, false);
    check_range(b, g, all, 0);
    for (int r : all) CHECK(b.valid(r) && b.slot(r) == r && !b.needs_refresh(r));
    check_book(b);

    // iteration 1.  The first trial starts over at slot 0 and so overwrites the iterates' planes: its rows are valid at the trial
    // point, and the one whose trial is rejected has nothing to go back to
    b.start_over();
    g = b.claim(all, true);
    check_range(b, g, all, 0);
    for (int r : all) CHECK(b.valid(r));
    b.reject_trial(0);
    CHECK(b.stale(0) && b.needs_refresh(0) && !b.valid(0));
    check_book(b);

    // a second trial of a few rows in the same iteration: a disjoint range behind the first; rejected, a row goes back to the
    // planes it had, which survive
    const std::vector<int> few = {3, 7, 8, (int)R - 1};
    const PlaneSlots::Range g2 = b.claim(few, true);
    check_range(b, g2, few, Rp);
    CHECK(g2.lo >= g.hi);
    for (int r : few) CHECK(b.valid(r) && b.slot(r) >= Rp);
    // ... a re-run of two of them keeps the slots they hold, within the enclosing tiles, and changes nothing
    {
        const Snapshot before(b);
        const std::vector<int> rerun = {7, (int)R - 1};
        const PlaneSlots::Range h = b.held(rerun);
        CHECK(h.slot[0] == g2.slot[1] && h.slot[1] == g2.slot[3]);
        CHECK(h.lo == Rp && h.hi == Rp + 32);
        CHECK(before == Snapshot(b) && b.held({7}).slot[0] == g2.slot[1]);
    }
    b.reject_trial(7);
    CHECK(b.valid(7) && b.slot(7) == 7 && !b.stale(7));
    CHECK(b.valid(3) && b.slot(3) == Rp); // (accepted: stays on the planes of the trial)
    check_book(b);

    // an objective-only trial runs in the scratch range and changes nothing but the slots of that pass
    {
        const Snapshot before(b);
        const std::vector<int> some = {1, 2, (int)R - 2};
        const PlaneSlots::Range s = b.scratch(some);
        CHECK(s.lo == Smain && s.hi == Smain + 32 && s.hi <= Scap);
        for (size_t a = 0; a < some.size(); ++a) CHECK(s.slot[a] == Smain + (int64_t)a && b.held({some[a]}).slot[0] == Smain + (int)a);
        CHECK(before == Snapshot(b));
        const PlaneSlots::Range h = b.held({2}); // (its re-run stays in the scratch range too)
        CHECK(h.slot[0] == Smain + 1 && h.lo == Smain && h.hi == Smain + 32 && before == Snapshot(b));
        const PlaneSlots::Range big = b.scratch(all);
        CHECK(big.lo == Smain && big.hi == Smain + Rp && big.hi <= Scap && before == Snapshot(b));
        // ... nor where the next claim goes: right behind the second trial
        const PlaneSlots::Range g3 = b.claim({1}, false);
        check_range(b, g3, {1}, Rp + 32);
        CHECK(b.valid(1) && b.slot(1) == Rp + 32);
    }
    check_book(b);

    // iteration 2: rows A, then the few rows B again and again until their range would cross Smain and starts over at slot 0.
    // Exactly the rows of A whose planes lay in the overwritten slots turn stale
    b.start_over();
    const int nA = (int)(R - R / 4), nB = (int)(R / 4);
    const std::vector<int> A = range(0, nA), B = range(nA, (int)R);
    const int64_t npA = round32(nA), npB = round32(nB);
    g = b.claim(A, false);
    check_range(b, g, A, 0);
    int64_t next = npA;
    bool wrapped = false;
    for (int i = 0; i < 64 && !wrapped; ++i) {
        const int64_t base = next + npB > Smain ? 0 : next; // (next is a multiple of 32 here)
        const PlaneSlots::Range gb = b.claim(B, false);
        check_range(b, gb, B, base);
        CHECK(gb.hi <= Smain);
        next = base + npB;
        wrapped = base == 0;
        for (int r : B) CHECK(b.valid(r));
        for (int r : A) {
            const bool overwritten = wrapped && r < npB; // (row r of A ran in slot r)
            CHECK(b.valid(r) == !overwritten && b.stale(r) == overwritten && b.slot(r) == (overwritten ? -1 : r));
        }
        check_book(b);
    }
    CHECK(wrapped);

    // a trial that overwrites the planes of its own iterate (the first row of B holds slot 0 now) and is rejected: stale
    {
        const int r = B[0];
        b.start_over();
        const PlaneSlots::Range t = b.claim({r}, true); // slot 0 again: the planes of its iterate are the ones it overwrites
        check_range(b, t, {r}, 0);
        b.reject_trial(r);
        CHECK(b.stale(r) && !b.valid(r));
    }
    check_book(b);

    // the last resort of the solver's refresh: from slot 0, a pass over every row that still needs one makes all of them valid
    b.mark_stale(5 % (int)R);
    b.start_over();
    g = b.claim(all, false);
    check_range(b, g, all, 0);
    for (int r : all) CHECK(b.valid(r) && !b.needs_refresh(r) && b.slot(r) == r);
    check_book(b);
}

// FP64 path: V is indexed by row; the book only records whether a row's V is current
static void fp64_convention() {
    const int64_t Rp = round32(R), Smain = Rp + 64, Scap = Smain + Rp;
    PlaneSlots b;
    CHECK(b.reset(R, Smain, Scap));
    const int r = (int)R - 1;
    CHECK(b.needs_refresh(r));
    b.set_row_indexed(r);
    CHECK(!b.needs_refresh(r) && b.slot(r) == 0 && !b.stale(r));
    b.mark_stale(r); // (every trial overwrites the row's V)
    CHECK(b.needs_refresh(r) && b.slot(r) == 0);
    b.set_row_indexed(r);
    CHECK(!b.needs_refresh(r) && b.slot(r) == 0);
    // a row that came over from the int8 passes keeps the slot it had
    b.claim({0, 1, 2}, false);
    b.mark_stale(2);
    b.set_row_indexed(2);
    CHECK(b.slot(2) == 2 && !b.needs_refresh(2));
}

int main(int argc, char **argv) {
    R = argc > 1 ? std::atoll(argv[1]) : 0;
    if (R < 16) {
        std::printf("usage: plane_slots R (R >= 16)\n");
        return 2;
    }
    int8_sequences(R / 2 > 96);
    fp64_convention();
    std::printf("ok\n");
    return 0;
}
