// CPU sweep of the coefficient tables K21 reads (activezero_amd/csrc/az_resample_table.h), built with
// g++ -fsanitize=address,undefined by tests/test_resample_table_cpu.py.  Exit code 0 = every property held.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../activezero_amd/csrc/az_resample_table.h"

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++fails < 20) { std::printf("FAIL %s:%d: %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const int32_t GUARD = 0x5a5a5a5a;
static const int32_t ONE = 1 << AZ_RESAMPLE_BITS;

// the table of (in, out) in a buffer of exactly its size plus one guard word; checks the properties every table has
static std::vector<int32_t> checked_table(int in, int out) {
    const int ks = az_resample_ksize(in, out);
    CHECK(ks >= 3 && ks <= AZ_RESAMPLE_MAX_KSIZE && (ks & 1), "%d -> %d: ksize %d", in, out, ks);
    if (ks < 0) return {};
    std::vector<int32_t> t((size_t)out * (2 + ks) + 1, GUARD);
    CHECK(az_resample_table(t.data(), in, out) == AZ_OK, "%d -> %d", in, out);
    CHECK(t.back() == GUARD, "%d -> %d: the word after the table was written", in, out);
    int prev_first = 0, prev_last = 0;
    for (int xx = 0; xx < out; ++xx) {
        const int32_t *row = t.data() + (size_t)xx * (2 + ks);
        const int first = row[0], count = row[1];
        CHECK(first >= 0 && count >= 1 && first + count <= in && count <= ks, "%d -> %d row %d: first %d count %d ksize %d",
              in, out, xx, first, count, ks);
        CHECK(first >= prev_first && first + count >= prev_last, "%d -> %d row %d: the taps move backwards", in, out, xx);
        prev_first = first; prev_last = first + count;
        long long sum = 0;
        for (int k = 0; k < ks; ++k) {
            CHECK(row[2 + k] >= 0, "%d -> %d row %d: coef[%d] = %d", in, out, xx, k, row[2 + k]);
            if (k >= count) CHECK(row[2 + k] == 0, "%d -> %d row %d: coef[%d] = %d beyond count %d", in, out, xx, k, row[2 + k], count);
            sum += row[2 + k];
        }
        // each entry is rounded separately: the sum is within count units of 2^22
        CHECK(sum >= ONE - count && sum <= ONE + count, "%d -> %d row %d: coefficients sum to %lld", in, out, xx, sum);
    }
    return t;
}

static void check_literal(int in, int out, int ks, const std::vector<std::vector<int32_t>> &rows) {
    const std::vector<int32_t> t = checked_table(in, out);
    CHECK(az_resample_ksize(in, out) == ks && (int)rows.size() == out, "%d -> %d: ksize", in, out);
    if (t.size() != (size_t)out * (2 + ks) + 1) return;
    for (int xx = 0; xx < out; ++xx)
        for (int e = 0; e < 2 + ks; ++e) {
            const int32_t want = e < (int)rows[xx].size() ? rows[xx][e] : 0;
            CHECK(t[(size_t)xx * (2 + ks) + e] == want, "%d -> %d row %d entry %d: %d, expected %d", in, out, xx, e,
                  t[(size_t)xx * (2 + ks) + e], want);
        }
}

int main() {
    // 1. every (in, out) up to 96 inside the ratio cap, and the two axes of the full-size resize
    int swept = 0;
    for (int in = 1; in <= 96; ++in)
        for (int out = 1; out <= 96; ++out)
            if (in <= AZ_RESAMPLE_MAX_RATIO * out) { checked_table(in, out); ++swept; }
    checked_table(720, 540);
    checked_table(1280, 960);
    CHECK(az_resample_ksize(720, 540) == 5 && az_resample_ksize(1280, 960) == 5, "full size: ksize");
    // 2. the known answers: first, count, then the non-zero coefficients
    check_literal(8, 6, 5, {{0, 2, 2936013, 1258291}, {1, 2, 2097152, 2097152}, {2, 3, 1143901, 2669103, 381300},
                            {3, 3, 381300, 2669103, 1143901}, {5, 2, 2097152, 2097152}, {6, 2, 1258291, 2936013}});
    check_literal(3, 5, 3, {{0, 1, 4194304}, {0, 2, 2516582, 1677722}, {1, 2, 4194304}, {1, 2, 1677722, 2516582},
                            {2, 1, 4194304}});
    // 3. the identity, the cap, and the refusals
    {
        const std::vector<int32_t> t = checked_table(540, 540);
        for (int xx = 0; xx < 540 && t.size() > 1; ++xx)
            CHECK(t[(size_t)xx * 5] == xx && t[(size_t)xx * 5 + 2] == ONE && t[(size_t)xx * 5 + 3] == 0 && t[(size_t)xx * 5 + 4] == 0,
                  "identity row %d", xx);  // one tap of 2^22 on the pixel itself (a second listed tap has weight zero)
    }
    CHECK(az_resample_ksize(64, 8) == 17 && az_resample_ksize(200, 25) == 17, "ksize at the cap");
    CHECK(az_resample_ksize(65, 8) == AZ_EUNSUPPORTED && az_resample_ksize(201, 25) == AZ_EUNSUPPORTED, "above the cap");
    for (int in = 9; in <= 17; ++in) checked_table(in, 1);  // a short axis is taken at any ratio, laid out with 17 taps
    CHECK(az_resample_ksize(13, 1) == 17 && az_resample_ksize(18, 2) == AZ_EUNSUPPORTED, "short axes");
    CHECK(az_resample_ksize(0, 8) == AZ_EINVAL && az_resample_ksize(8, 0) == AZ_EINVAL && az_resample_ksize(-3, 8) == AZ_EINVAL &&
          az_resample_ksize(8, -1) == AZ_EINVAL, "non-positive sizes");
    {
        int32_t word = GUARD;
        CHECK(az_resample_table(&word, 65, 8) == AZ_EUNSUPPORTED && az_resample_table(&word, 0, 8) == AZ_EINVAL &&
              az_resample_table(nullptr, 8, 6) == AZ_EINVAL && word == GUARD, "refusals write nothing");
    }
    std::printf("resample tables: %d size pairs swept, %d failures\n", swept, fails);
    return fails ? 1 : 0;
}
