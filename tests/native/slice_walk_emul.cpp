// Host emulation of the flattened slice walk (csrc/slice_walk.hpp) over the arithmetic the device uses (csrc/slice_walk_core.hpp): the
// 64 lanes of a wave are arrays, a shuffle is an index.  A set of slices is walked EPW at a time, as the kernels do, and every
// flattened position reports the slice and the absolute index it was given; a hit pattern over the elements is counted per slice
// through the step masks.  tests/test_slice_walk_core_cpu.py compares both with the plain concatenation of the slices.
// Also here: the pick key and the stop rule of the gather rounds (csrc/gather_key.hpp).
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../../sourmash_amd/csrc/slice_walk_core.hpp"
#include "../../sourmash_amd/csrc/gather_key.hpp"

namespace {

constexpr int LANES = 64;

// wave_incl_sum<WIDTH> of slice_walk.hpp, lane by lane: __shfl_up(v, d) hands lane l the value of lane l - d (its own below d)
template <int WIDTH>
void incl_sum(uint32_t (&v)[LANES]) {
    for (int d = 1; d < WIDTH; d <<= 1) {
        uint32_t o[LANES];
        for (int l = 0; l < LANES; ++l) o[l] = v[l >= d ? l - d : l];
        for (int l = 0; l < LANES; ++l)
            if (l >= d) v[l] += o[l];
    }
}

struct Out {
    uint32_t* slice;
    uint64_t* index;
    uint64_t cap, n = 0;
    bool overflow = false;
    void put(uint32_t s, uint64_t i) {
        if (n < cap) { slice[n] = s; index[n] = i; }
        else overflow = true;
        ++n;
    }
};

// SliceGroup<EPW>::build, then the walk of a kernel that keeps `ahead` steps of 64 in flight (lanes past the end take the last
// element and discard it), then hits_of_step for every step
template <int EPW>
void walk_group(const uint64_t* lo, const uint32_t* n, uint32_t first_slice, uint32_t n_slices, const uint8_t* hit, int ahead, Out& out,
                uint64_t* hits_out) {
    uint32_t incl[LANES], cnt[LANES], excl[LANES];
    uint64_t start[LANES];
    for (int l = 0; l < LANES; ++l) {
        const bool mine = l < EPW && first_slice + (uint32_t)l < n_slices;
        cnt[l] = mine ? n[first_slice + l] : 0u;
        start[l] = mine ? lo[first_slice + l] : 0u;
        incl[l] = cnt[l];
    }
    incl_sum<EPW>(incl);
    const uint32_t total = incl[EPW - 1];
    uint32_t bound[EPW - 1];
    for (int k = 0; k < EPW - 1; ++k) bound[k] = incl[k];
    for (int l = 0; l < LANES; ++l) excl[l] = incl[l] - cnt[l];
    uint32_t row_hits[LANES] = {};
    const uint64_t base = out.n;                                    // where this group's elements begin in the concatenation
    for (uint32_t t0 = 0; t0 < total; t0 += 64u * (uint32_t)ahead)
        for (int u = 0; u < ahead; ++u) {
            const uint32_t tb = t0 + 64u * (uint32_t)u;
            unsigned long long ballot = 0;
            for (int lane = 0; lane < LANES; ++lane) {
                const uint32_t t = tb + (uint32_t)lane;
                const bool ok = t < total;
                const uint32_t tt = ok ? t : total - 1;
                const int h = smg::slice_of<EPW>(tt, bound);
                const uint64_t at = start[h] + (tt - excl[h]);      // the three shuffles of SliceGroup::at
                if (!ok) continue;
                out.put(first_slice + (uint32_t)h, at);
                if (hit[base + t]) ballot |= 1ull << lane;
            }
            for (int l = 0; l < EPW; ++l) row_hits[l] += (uint32_t)__builtin_popcountll(ballot & smg::slice_step_mask(excl[l], incl[l], tb));
        }
    for (int l = 0; l < EPW; ++l)
        if (first_slice + (uint32_t)l < n_slices) hits_out[first_slice + l] = row_hits[l];
}

template <int EPW>
int64_t walk(const uint64_t* lo, const uint32_t* n, uint32_t n_slices, const uint8_t* hit, int ahead, Out& out, uint64_t* hits_out) {
    for (uint32_t s = 0; s < n_slices; s += EPW) walk_group<EPW>(lo, n, s, n_slices, hit, ahead, out, hits_out);
    return out.overflow ? -1 : (int64_t)out.n;
}

}  // namespace

// Walks slices [lo[s], lo[s] + n[s]), epw (2 or 16) at a time.  hit: one byte per element of the concatenation (`cap` of them).
// out_slice / out_index [cap]: what every flattened position was given, in walk order; out_hits [n_slices].  Returns the number of
// positions walked, -1 when that is more than cap, -2 for an epw the kernels do not use.
extern "C" int64_t emul_slice_walk(int epw, const uint64_t* lo, const uint32_t* n, uint32_t n_slices, const uint8_t* hit, uint64_t cap, int ahead,
                                   uint32_t* out_slice, uint64_t* out_index, uint64_t* out_hits) {
    Out out{out_slice, out_index, cap};
    if (epw == 2) return walk<2>(lo, n, n_slices, hit, ahead, out, out_hits);
    if (epw == 16) return walk<16>(lo, n, n_slices, hit, ahead, out, out_hits);
    return -2;
}

extern "C" uint64_t emul_gather_key(uint64_t count, uint64_t global_index) { return smg::gather_key(count, global_index); }
extern "C" uint64_t emul_gather_key_index(uint64_t key) { return smg::gather_key_index(key); }
extern "C" int emul_gather_stops(uint64_t key, uint64_t qlen, uint64_t thr) { return smg::gather_stops(key, qlen, thr) ? 1 : 0; }

#if defined(SLICE_WALK_EMUL_MAIN)
// A program of its own, for a build with -fsanitize=address,undefined (a shift by 64 in a step mask would stop it): slice sets with
// the group totals 0 .. 300 and a few long ones, for both widths and both depths, against the concatenation, vectors sized exactly.
int main() {
    uint64_t sets = 0, positions = 0, rng = 0x9e3779b97f4a7c15ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    for (int epw : {2, 16})
        for (int ahead : {1, 4})
            for (uint32_t total = 0; total <= 1100; total += (total < 300 ? 1 : 199)) {
                // three groups: the total cut at random places (empty slices included), nothing, one slice holding everything
                std::vector<uint32_t> n;
                uint32_t left = total;
                for (int l = 0; l < epw - 1; ++l) {
                    const uint32_t take = next() % 3 == 0 ? 0u : (uint32_t)(next() % (left + 1));
                    n.push_back(take);
                    left -= take;
                }
                n.push_back(left);
                for (int l = 0; l < epw; ++l) n.push_back(0);
                n.push_back(total);
                std::vector<uint64_t> lo(n.size());
                for (size_t s = 0; s < n.size(); ++s) lo[s] = (s % 2 ? (1ull << 32) - 5 : 0ull) + 5000ull * s;
                std::vector<uint8_t> hit(2 * (size_t)total);
                for (auto& b : hit) b = next() & 1;
                std::vector<uint32_t> got_slice(hit.size());
                std::vector<uint64_t> got_index(hit.size()), got_hits(n.size(), ~0ull);
                const int64_t r = emul_slice_walk(epw, lo.data(), n.data(), (uint32_t)n.size(), hit.data(), hit.size(), ahead, got_slice.data(),
                                                  got_index.data(), got_hits.data());
                bool bad = r != (int64_t)hit.size();
                size_t f = 0;
                for (size_t s = 0; s < n.size() && !bad; ++s) {
                    uint64_t want_hits = 0;
                    for (uint32_t o = 0; o < n[s]; ++o, ++f) {
                        bad |= got_slice[f] != s || got_index[f] != lo[s] + o;
                        want_hits += hit[f];
                    }
                    bad |= got_hits[s] != want_hits;
                }
                if (bad) { printf("epw %d, %d steps in flight, total %u: the walk is not the concatenation\n", epw, ahead, total); return 1; }
                ++sets;
                positions += hit.size();
            }
    if (smg::gather_key_index(smg::gather_key(1, 0)) != 0 || smg::gather_key_index(smg::gather_key(7, 0xffffffffull)) != 0xffffffffull ||
        smg::gather_key(5, 3) <= smg::gather_key(5, 4) || smg::gather_key(6, 4) <= smg::gather_key(5, 3) || !smg::gather_stops(0, 9, 0) ||
        smg::gather_stops(smg::gather_key(3, 1), 9, 3)) {
        printf("the pick key or the stop rule is wrong\n");
        return 1;
    }
    printf("ok: %llu slice sets, %llu positions\n", (unsigned long long)sets, (unsigned long long)positions);
    return 0;
}
#endif
