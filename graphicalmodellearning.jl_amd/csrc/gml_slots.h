// The slot book of the solver's int8-limb workspace (gml_solver_impl.h: Solver::slots): which row owns which V planes.
//
// A pass evaluates its rows in consecutive slots of the workspace and leaves each row's V planes (the fixed-point weights the
// Hessians and the Hessian-vector products read) in the row's slot.  The slots are [0, Smain) -- the main range, whose planes
// feed the curvature -- and [Smain, Scap) -- a scratch range for objective-only trials, whose planes nobody reads.  The passes
// of one iteration claim disjoint ranges of the main one, one after the other; when the next range would cross Smain the claims
// start over at slot 0, and a row whose planes are overwritten that way is STALE: it needs a fresh pass before it may enter a
// Hessian (needs_refresh, valid).  A trial pass remembers the planes of the iterate it started from, so that a rejected trial can
// go back to them if they survived.
//
// Plain C++17 with no device header: tests/native/plane_slots.cpp drives it on the host alone.
#pragma once
#include <algorithm>
#include <cassert>
#include <cstdint>
#include <vector>

namespace gml {

class PlaneSlots {
  public:
    // the slots of one pass: [lo, hi) is the range it sweeps (multiples of 32), slot[a] the slot of its a-th row
    struct Range {
        int64_t lo = 0, hi = 0;
        std::vector<int64_t> slot;
    };

    // R rows, Smain main slots, Scap slots in all.  What makes the wrap of claim() safe: a pass lists every row at most once, so its
    // n <= R rows take round_up(n, 32) <= round_up(R, 32) <= Smain slots -- a range that starts over at slot 0 always fits below
    // Smain and never overlaps itself; the scratch range holds as many.  false: the sizes break that (the book is unusable).
    bool reset(int64_t R, int64_t Smain, int64_t Scap) {
        Smain_ = Smain;
        Scap_ = Scap;
        slot_next = 0;
        vslot.assign((size_t)R, -1);
        vprev.assign((size_t)R, -1);
        pslot.assign((size_t)R, -1);
        vstale.assign((size_t)R, 0);
        owner.assign((size_t)std::max<int64_t>(Scap, 0), -1);
        return R >= 0 && round32(R) <= Smain && Smain + round32(R) <= Scap;
    }
    int64_t capacity() const { return Scap_; }

    // a fresh consecutive range of the main slots for a pass whose V planes are kept.  at_trial: the rows are evaluated at a trial
    // point; each remembers the planes of its iterate for reject_trial
    Range claim(const std::vector<int> &rows, bool at_trial) {
        const int64_t n = (int64_t)rows.size(), np = round32(n);
        assert(np <= Smain_); // (the invariant of reset)
        int64_t base = round32(slot_next);
        if (base + np > Smain_) base = 0; // wrap: the rows whose V planes are overwritten become stale below
        slot_next = base + np;
        Range g{base, base + np, std::vector<int64_t>((size_t)n)};
        for (int64_t a = 0; a < np; ++a) {
            const int64_t s = base + a;
            const int prev = owner[s];
            if (prev >= 0 && vslot[prev] == s) {
                vslot[prev] = -1;
                vstale[prev] = 1;
            }
            owner[s] = a < n ? rows[a] : -1;
        }
        for (int64_t a = 0; a < n; ++a) {
            const int r = rows[a];
            g.slot[a] = base + a;
            vprev[r] = at_trial ? vslot[r] : -1; // a rejected trial goes back to the planes of the iterate, if they survive
            vslot[r] = (int)(base + a);
            vstale[r] = 0;
            pslot[r] = (int)(base + a);
        }
        return g;
    }
    // objective-only trial: scratch slots, the rows keep the V planes of their iterates
    Range scratch(const std::vector<int> &rows) {
        const int64_t n = (int64_t)rows.size(), np = round32(n);
        assert(Smain_ + np <= Scap_);
        Range g{Smain_, Smain_ + np, std::vector<int64_t>((size_t)n)};
        for (int64_t a = 0; a < n; ++a) pslot[rows[a]] = (int)(g.slot[a] = Smain_ + a);
        return g;
    }
    // re-run of some rows of the last pass (a tighter scale): the slots those rows already hold -- a re-run must not claim new
    // slots, it could wrap around and overwrite planes of its own pass.  [lo, hi): the tiles of 32 that enclose them
    Range held(const std::vector<int> &rows) const {
        Range g{Scap_, 0, std::vector<int64_t>(rows.size())};
        for (size_t a = 0; a < rows.size(); ++a) {
            g.slot[a] = pslot[rows[a]];
            g.lo = std::min(g.lo, g.slot[a] / 32 * 32);
            g.hi = std::max(g.hi, g.slot[a] / 32 * 32 + 32);
        }
        return g;
    }
    // the trial that claim(.., true) evaluated for row r was rejected: the planes just written belong to the rejected point -- back
    // to those of the iterate, if they survive
    void reject_trial(int r) {
        const int pv = vprev[r];
        if (pv >= 0 && owner[pv] == r) vslot[r] = pv;
        else vstale[r] = 1;
    }
    void mark_stale(int r) { vstale[r] = 1; }
    // the FP64 path keeps V [row][Kp] indexed by row: a pass there makes the row's V current, slot 0 stands for "has one"
    void set_row_indexed(int r) {
        vstale[r] = 0;
        if (vslot[r] < 0) vslot[r] = 0;
    }
    // the next claim starts at slot 0.  At the start of an iteration: the V planes of the previous one's passes are no longer needed;
    // as the last resort of a refresh: a pass over every active row then leaves all of them valid (they always fit)
    void start_over() { slot_next = 0; }

    int slot(int r) const { return vslot[r]; }        // of row r's V planes, or -1
    bool stale(int r) const { return vstale[r] != 0; }
    int slot_owner(int r) const { return in_range(vslot[r]) ? owner[vslot[r]] : -2; } // who owns the slot row r points at (-2: none)
    int owner_of(int64_t s) const { return owner[s]; }
    bool needs_refresh(int r) const { return vstale[r] || vslot[r] < 0; }
    // row r may enter a Hessian: it points at a slot of the workspace that it still owns, and its planes are current
    bool valid(int r) const { return in_range(vslot[r]) && owner[vslot[r]] == r && !vstale[r]; }

  private:
    static int64_t round32(int64_t a) { return (a + 31) / 32 * 32; }
    bool in_range(int s) const { return s >= 0 && s < Scap_; }
    int64_t Smain_ = 0, Scap_ = 0, slot_next = 0;
    std::vector<int> vslot, vprev, owner, pslot; // by row: slot of the V planes, of the iterate's (trial), of the last pass; by slot: the row
    std::vector<uint8_t> vstale;
};

} // namespace gml
