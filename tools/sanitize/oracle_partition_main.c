/* Stand-alone check of the CPU oracle's Partition at the ends of int64, meant to be built with
 *   gcc -std=c11 -fopenmp -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all oracle_partition_main.c
 * (tests/test_int64_edges_cpu.py does; a plain build still checks the values).
 *
 * bucket_of once returned the wrapped difference x - from as the bucket: with x - from >= 2^63 that is a negative index into
 * the counting sort's table (a heap write before the allocation) or a negative key of the sort.  The program runs Partition
 * through the oracle's own entry points -- orc_add_column, orc_run, orc_output -- over data drawn from the edge pool and pivots
 * RangeC pmin count 1 at both ends, and compares every result with a ranking computed here in 128-bit arithmetic.
 * Prints "ok <programs>" and exits 0, or says what differed and exits 1. */
#include "../../oracle/vdl_oracle.c"

#define I64_MIN INT64_MIN
#define I64_MAX INT64_MAX

static const int64_t POOL[] = {
    I64_MIN, I64_MIN + 1, I64_MIN + 2, I64_MAX, I64_MAX - 1, I64_MAX - 2, (int64_t)1 << 62, -((int64_t)1 << 62),
    ((int64_t)1 << 31) - 1, (int64_t)1 << 31, ((int64_t)1 << 31) + 1, -((int64_t)1 << 31) - 1, -((int64_t)1 << 31), -((int64_t)1 << 31) + 1,
    ((int64_t)1 << 32) - 1, (int64_t)1 << 32, ((int64_t)1 << 32) + 1, -((int64_t)1 << 32) - 1, -((int64_t)1 << 32), -((int64_t)1 << 32) + 1,
    63, 64, 65, -63, -64, -65, -2, -1, 0, 1, 2 };
enum { NPOOL = (int)(sizeof POOL / sizeof POOL[0]) };

/* bucket 0 for x <= pmin, else min(x - pmin, count): exact, no wrap */
static __int128 exact_bucket(int64_t x, int64_t pmin, int64_t count) {
    if (x <= pmin) return 0;
    __int128 b = (__int128)x - (__int128)pmin;
    return b < (__int128)count ? b : (__int128)count;
}

/* rank of every slot by (bucket, slot): O(n^2), n is small */
static void exact_ranks(const int64_t *x, int n, int64_t pmin, int64_t count, int64_t *rank) {
    for (int i = 0; i < n; i++) {
        int64_t r = 0;
        const __int128 bi = exact_bucket(x[i], pmin, count);
        for (int j = 0; j < n; j++) {
            const __int128 bj = exact_bucket(x[j], pmin, count);
            if (bj < bi || (bj == bi && j < i)) r++;
        }
        rank[i] = r;
    }
}

static int programs = 0;

/* Partition(t.x, RangeC pmin count 1) through the oracle; 0 if it equals `want` */
static int check(const int64_t *x, int n, int64_t pmin, int64_t count, const int64_t *want, const char *what) {
    orc_ctx *c = orc_open();
    if (orc_add_column(c, "t.x", x, 8, n)) { printf("%s: add_column: %s\n", what, orc_last_error(c)); return 1; }
    char text[512];
    const int len = snprintf(text, sizeof text,
        "1,Load,t.x\n2,Project,val,Id 1,x\n3,RangeC,val,%lld,%lld,1\n4,Partition,val,Id 2,val,Id 3,val\n5,MaterializeCompact,Id 4\n",
        (long long)pmin, (long long)count);
    if (orc_run(c, text, (size_t)len)) { printf("%s: run: %s\n", what, orc_last_error(c)); return 1; }
    const char *name, *tmp; const int64_t *vals; int64_t m = 0;
    if (orc_n_outputs(c) != 1 || orc_output(c, 0, &name, &tmp, &vals, &m) || m != n) { printf("%s: %lld values for %d rows\n", what, (long long)m, n); return 1; }
    int bad = 0;
    for (int i = 0; i < n && !bad; i++)
        if (vals[i] != want[i]) { printf("%s (pmin %lld count %lld): slot %d (value %lld) goes to %lld, expected %lld\n", what, (long long)pmin, (long long)count, i, (long long)x[i], (long long)vals[i], (long long)want[i]); bad = 1; }
    orc_close(c);
    programs++;
    return bad;
}

int main(void) {
    int bad = 0;
    /* the two cases that showed the defect: the counting sort, and the sort of (bucket, slot) pairs */
    {
        const int64_t x[] = { 5, I64_MAX, 9, -100, 1000, I64_MAX - 1 }, want[] = { 1, 2, 3, 0, 4, 5 };
        bad |= check(x, 6, -5, 10, want, "counting sort");
    }
    {
        const int64_t x[] = { 5, I64_MAX, 9, I64_MIN, 1000 }, want[] = { 1, 4, 2, 0, 3 };
        bad |= check(x, 5, -5, (int64_t)1 << 30, want, "pair sort");
    }
    /* the pool, in three orders, against every pivot start and count of the edge tests */
    static const int64_t PMIN[] = { I64_MIN, I64_MIN + 1, -5, 0, I64_MAX - 3 };
    static const int64_t COUNT[] = { 1, 10, 255, 256, (int64_t)1 << 30, (int64_t)1 << 40, (int64_t)1 << 62 };
    int64_t x[2 * NPOOL], want[2 * NPOOL];
    for (int order = 0; order < 3; order++) {
        for (int i = 0; i < 2 * NPOOL; i++)
            x[i] = order == 0 ? POOL[i % NPOOL] : order == 1 ? POOL[(2 * NPOOL - 1 - i) % NPOOL] : POOL[(int)(((unsigned)i * 7u + 3u) % NPOOL)];
        for (size_t p = 0; p < sizeof PMIN / sizeof PMIN[0]; p++)
            for (size_t k = 0; k < sizeof COUNT / sizeof COUNT[0]; k++) {
                exact_ranks(x, 2 * NPOOL, PMIN[p], COUNT[k], want);
                bad |= check(x, 2 * NPOOL, PMIN[p], COUNT[k], want, "pool");
            }
    }
    if (bad) return 1;
    printf("ok %d\n", programs);
    return 0;
}
