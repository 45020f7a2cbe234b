// many_core.hpp compiled for the host: the rules of the many-queries pass behind a C interface (tests/test_many_core_cpu.py).
#include "../../sourmash_amd/csrc/many_core.hpp"

using namespace smg;

extern "C" {

uint32_t emul_many_block() { return MANY_BLOCK; }
uint32_t emul_many_q_block() { return MANY_Q_BLOCK; }
uint32_t emul_many_q_block_max() { return MANY_Q_BLOCK_MAX; }

uint64_t emul_many_cutoff(uint64_t a, uint64_t b) { return many_cutoff(a, b); }
uint64_t emul_many_cut_len(const uint64_t* row, uint64_t n, uint64_t cutoff) { return many_cut_len(row, n, cutoff); }

// ab[0], ab[1]: the range in, the narrowed range out
void emul_many_post_range(const uint32_t* post, uint32_t* ab, uint32_t q_lo, uint32_t q_hi) { many_post_range(post, &ab[0], &ab[1], q_lo, q_hi); }

uint64_t emul_many_key(uint32_t q, uint32_t row) { return many_key(q, row); }
uint32_t emul_many_key_query(uint64_t key) { return many_key_query(key); }
uint32_t emul_many_key_row(uint64_t key) { return many_key_row(key); }

uint32_t emul_many_need(uint32_t mode, double threshold, uint64_t n_q) { return many_need(mode, threshold, n_q); }

// params: ksize, hash_function, seed, max_hash, num of each side
uint32_t emul_many_compat_code(const uint64_t* a, const uint64_t* b) {
    return many_compat_code(ManyParams{(uint32_t)a[0], (uint32_t)a[1], a[2], a[3], a[4]}, ManyParams{(uint32_t)b[0], (uint32_t)b[1], b[2], b[3], b[4]});
}

// The whole pass as the kernel walks it, one query block at a time, on the host: counts[q_block] per row, hits appended in
// (block, row, query) order.  -> hits found; out_* hold the first `capacity`.
uint64_t emul_many_pass(const uint64_t* U, const uint32_t* uoff, const uint32_t* post, uint64_t n_u, const uint64_t* hashes, const uint64_t* offsets,
                        uint64_t n_rows, uint64_t cutoff, const uint32_t* need, uint32_t m, uint32_t q_block, uint32_t* out_q, uint32_t* out_row,
                        uint32_t* out_cnt, uint64_t capacity, uint32_t* counters) {
    uint64_t hits = 0;
    for (uint32_t q_lo = 0; q_lo < m; q_lo += q_block) {
        const uint32_t qb = m - q_lo < q_block ? m - q_lo : q_block;
        for (uint64_t r = 0; r < n_rows; ++r) {
            for (uint64_t i = offsets[r]; i < offsets[r + 1]; ++i) {
                const uint64_t h = hashes[i];
                if (h > cutoff) break;
                const uint64_t j = many_cut_len(U, n_u, h);            // entries <= h: h itself is the last of them, if present
                if (j == 0 || U[j - 1] != h) continue;
                uint32_t a = uoff[j - 1], b = uoff[j];
                many_post_range(post, &a, &b, q_lo, q_lo + qb);
                for (uint32_t p = a; p < b; ++p) ++counters[post[p] - q_lo];
            }
            for (uint32_t i = 0; i < qb; ++i) {
                const uint32_t c = counters[i];
                counters[i] = 0;
                if (c != 0 && c >= need[q_lo + i]) {
                    if (hits < capacity) { out_q[hits] = q_lo + i; out_row[hits] = (uint32_t)r; out_cnt[hits] = c; }
                    ++hits;
                }
            }
        }
    }
    return hits;
}

}  // extern "C"
