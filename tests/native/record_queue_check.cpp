// Stand-alone check of csrc/record_queue.hpp (plain g++, no HIP): the valid-prefix rule against a direct restatement of the
// reference's streaming walk (signature.rs:38-58 + :246-306: k-mer after k-mer; the first one that holds a byte outside ACGTacgt
// stops the walk, every k-mer before it has been added), the append and the release rule.
//   g++ -O1 -std=c++17 -Wall -Werror -o record_queue_check record_queue_check.cpp && ./record_queue_check
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../sourmash_amd/csrc/record_queue.hpp"

using namespace smg;

static long n_cases = 0;
#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "FAILED %s (line %d): ", #cond, __LINE__);        \
            fprintf(stderr, __VA_ARGS__);                                     \
            fprintf(stderr, "\n");                                            \
            exit(1);                                                          \
        }                                                                     \
    } while (0)

static bool valid_base(uint8_t c) { return memchr("ACGTacgt", c, 8) != nullptr && c != 0; }

// the reference's walk: -> number of k-mers added; *stopped: the walk met a bad k-mer (its index is the return value)
static size_t walk(const std::vector<uint8_t>& s, size_t k, bool force, bool* stopped) {
    *stopped = false;
    size_t added = 0;
    for (size_t i = 0; i + k <= s.size(); ++i) {
        bool ok = true;
        for (size_t j = 0; j < k; ++j) ok = ok && valid_base(s[i + j]);
        if (!ok && !force) { *stopped = true; return i; }
        ++added;                                                    // (force: the kernel skips the k-mer; the record is queued whole)
    }
    return added;
}

static size_t naive_first_invalid(const std::vector<uint8_t>& s) {
    for (size_t i = 0; i < s.size(); ++i)
        if (!valid_base(s[i])) return i;
    return SIZE_MAX;
}

static void check_record(const std::vector<uint8_t>& s, size_t k) {
    const size_t len = s.size();
    const size_t first_bad = naive_first_invalid(s);
    CHECK(first_invalid_byte(s.data(), len) == first_bad, "first_invalid_byte, len %zu", len);
    for (int force = 0; force < 2; ++force)
        for (int scanned = 0; scanned < 2; ++scanned) {
            bool stopped = false;
            const size_t kept = walk(s, k, force != 0, &stopped);
            const ValidPrefix v = scanned ? valid_prefix(s.data(), len, k, force != 0, true, first_bad) : valid_prefix(s.data(), len, k, force != 0);
            ++n_cases;
            CHECK(v.raise == stopped, "raise: k %zu len %zu bad %zu force %d scanned %d", k, len, first_bad, force, scanned);
            CHECK(v.use_len <= len, "use_len beyond the record: k %zu len %zu bad %zu", k, len, first_bad);
            if (!stopped) {
                CHECK(v.use_len == len, "a record that does not raise is queued whole: k %zu len %zu bad %zu force %d", k, len, first_bad, force);
                CHECK(kept == len - k + 1, "walk");
            } else {
                CHECK(v.bad_kmer == kept, "k-mer named: k %zu len %zu bad %zu: %zu, walk %zu", k, len, first_bad, v.bad_kmer, kept);
                CHECK(v.bad_kmer + k <= len, "the named k-mer lies in the record");
                CHECK(v.use_len == kept + (k - 1), "prefix: k %zu len %zu bad %zu: %zu for %zu k-mers", k, len, first_bad, v.use_len, kept);
            }
            // what reaches the queue holds exactly the walk's k-mers, and the separator
            std::string q = "ACGT\n";
            const bool due = queue_record(q, s.data(), v.use_len, k);
            CHECK(!due, "a short queue is not due");
            const size_t queued_kmers = v.use_len >= k ? v.use_len - k + 1 : 0;
            CHECK(queued_kmers == kept, "queued k-mers: %zu, walk %zu", queued_kmers, kept);
            if (kept == 0) CHECK(q == "ACGT\n", "nothing to queue");
            else CHECK(q.size() == 5 + v.use_len + 1 && q.back() == '\n' && memcmp(q.data() + 5, s.data(), v.use_len) == 0, "queued bytes");
        }
}

static void check_prefixes() {
    const size_t ks[] = {1, 2, 3, 21, 31, 32};
    const uint8_t bads[] = {'N', 'n', 0x00, 0xc1 /* 'A' with the top bit */, '\n'};
    const char fill[] = "ACGTacgtTGCAtgca";
    for (size_t k : ks) {
        const size_t lens[] = {k, k + 1, 2 * k - 1, 2 * k, 2 * k + 1};
        for (size_t len : lens) {
            std::vector<uint8_t> s(len);
            for (size_t i = 0; i < len; ++i) s[i] = (uint8_t)fill[(i * 7 + k) % 16];
            check_record(s, k);                                     // no bad byte
            for (size_t p = 0; p < len; ++p)
                for (uint8_t b : bads) {
                    std::vector<uint8_t> t = s;
                    t[p] = b;
                    check_record(t, k);
                    if (p + 2 < len) { t[len - 1] = 'N'; check_record(t, k); }   // a second bad byte behind the first changes nothing
                }
        }
    }
}

static void check_flush_threshold() {
    const std::string rec(150, 'A');
    std::string q(PENDING_FLUSH_BYTES - 152, 'C');
    CHECK(!queue_record(q, (const uint8_t*)rec.data(), rec.size(), 21) && q.size() == PENDING_FLUSH_BYTES - 1, "one byte short of the threshold");
    CHECK(queue_record(q, (const uint8_t*)rec.data(), rec.size(), 21), "at the threshold the queue is due");
    std::string r(PENDING_FLUSH_BYTES - 151, 'C');
    CHECK(queue_record(r, (const uint8_t*)rec.data(), rec.size(), 21) && r.size() == PENDING_FLUSH_BYTES, "exactly the threshold");
    n_cases += 3;
}

static void check_release() {
    const size_t mib = (size_t)1 << 20;
    CHECK(PENDING_KEEP_BYTES == mib && PENDING_FLUSH_BYTES == 32 * mib, "constants");
    // capacities on both sides of PENDING_KEEP_BYTES, as this standard library gives them: reserve(n) may give more than n, so
    // the low side is the largest request whose capacity is still at most 1 MiB, and every expectation is derived from the
    // capacity read back
    size_t low = mib;
    while (low > 0 && [&] { std::string t; t.reserve(low); return t.capacity() > mib; }()) low -= low > 4096 ? 4096 : 1;
    CHECK(low > mib / 2, "no request near 1 MiB gives a capacity of at most 1 MiB (last tried %zu)", low);
    for (size_t want : {low, mib + 1})
        for (int streaming = 0; streaming < 2; ++streaming) {
            std::string q;
            q.reserve(want);
            const size_t cap = q.capacity();
            CHECK(want == low ? cap <= mib : cap > mib, "reserve(%zu) gave %zu: the wrong side of 1 MiB", want, cap);
            q.assign(1000, 'A');
            release_queue(q, streaming != 0);
            ++n_cases;
            CHECK(q.empty(), "released queue is empty");
            if (streaming || cap <= mib) CHECK(q.capacity() == cap, "storage kept: cap %zu streaming %d -> %zu", cap, streaming, q.capacity());
            else CHECK(q.capacity() < cap && q.capacity() <= std::string().capacity(), "storage given back: cap %zu -> %zu", cap, q.capacity());
        }
}

int main() {
    check_prefixes();
    check_flush_threshold();
    check_release();
    printf("record queue ok: %ld cases\n", n_cases);
    return 0;
}
