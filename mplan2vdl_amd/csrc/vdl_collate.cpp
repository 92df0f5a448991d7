// vdl_collate.cpp -- collation indexes of string heaps: the build (kernels: vdl_collate.hip), the order step's text keys, and the
// device-free formulation vdl_collate_host.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "vdl.h"
#include "vdl_engine_internal.h"

namespace vdl {
namespace eng {

namespace {

struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

// The index of one heap column.  steps (may be null): device time of each step, by name.
std::shared_ptr<Collation> collation_build(vdl_ctx *c, const std::string &name, const Column &col, std::vector<Timing> *steps) {
    if (col.width != 1)
        throw Error(VDL_ERR_ARG, "collation: '" + name + "' is no string heap: a heap has one byte per slot, this column has " + std::to_string(col.width));
    const int64_t n = col.n;
    if (n >= ((int64_t)1 << 31)) throw Error(VDL_ERR_UNSUPPORTED, "collation: heap '" + name + "' has " + std::to_string(n) + " bytes; ranks are kept in 32 bits, for heaps below 2^31 bytes");
    hipStream_t s = c->stream;
    auto co = std::make_shared<Collation>();
    co->heap_n = n;
    if (n == 0) return co;
    const int8_t *heap = (const int8_t *)col.dev;

    std::vector<std::pair<const char *, hipEvent_t>> marks;
    struct Cleanup { std::vector<std::pair<const char *, hipEvent_t>> &m; ~Cleanup() { for (auto &e : m) (void)hipEventDestroy(e.second); } } cleanup{marks};
    auto mark = [&](const char *what) {
        if (!steps) return;
        hipEvent_t e = nullptr;
        HIP_CHECK(hipEventCreate(&e));
        marks.push_back({what, e});
        HIP_CHECK(hipEventRecord(e, s));
    };
    mark("");

    // 1. the starts: bitmap by ballots, population and offset list by the compaction every MaterializeCompact uses
    const int64_t nb = (n + compact_tile() - 1) / compact_tile(), nw = nb * (compact_tile() / 64);
    BufP starts = dev_alloc(c, sizeof(uint64_t) * (size_t)nw);
    HIP_CHECK(launch_fill_words((uint64_t *)starts->p, 0, nw, s));
    HIP_CHECK(launch_collate_mark(heap, n, (uint64_t *)starts->p, s));
    mark("Mark");
    BufP counts = dev_alloc(c, sizeof(int64_t) * (size_t)(nb + 1));
    HIP_CHECK(launch_compact_offsets((const uint64_t *)starts->p, n, (int64_t *)counts->p, s));
    int64_t d = 0;
    c->fetch_to_host((const int64_t *)counts->p + nb, 1, &d, s);
    if (d < 0 || d > (n + 1) / 2) throw Error(VDL_ERR_DEVICE, "internal: collation of '" + name + "' counted " + std::to_string(d) + " starts in " + std::to_string(n) + " bytes");
    co->strings = d;
    BufP off, perm, ranks;
    if (d > 0) {
        off = dev_alloc(c, sizeof(int64_t) * (size_t)d);
        Src iota; iota.kind = SRC_RANGE; iota.from = 0; iota.step = 1;
        HIP_CHECK(launch_compact_write(iota, (const uint64_t *)starts->p, n, (const int64_t *)counts->p, (int64_t *)off->p, s));
        BufP st = dev_alloc(c, sizeof(uint64_t) * kOrdStateHead);
        uint64_t *stw = (uint64_t *)st->p;
        HIP_CHECK(hipMemsetAsync(stw, 0, 2 * sizeof(uint64_t), s));
        HIP_CHECK(launch_collate_lengths(heap, n, (const int64_t *)off->p, d, stw, s));
        int64_t lw[2];
        c->fetch_to_host(stw, 2, lw, s);
        mark("Starts");
        if (lw[0] < 1 || lw[0] > n) throw Error(VDL_ERR_DEVICE, "internal: collation of '" + name + "' measured a longest string of " + std::to_string(lw[0]) + " bytes");
        if (lw[0] > kCollateMaxBytes)
            throw Error(VDL_ERR_UNSUPPORTED, "collation: heap '" + name + "' holds a string of " + std::to_string(lw[0]) + " bytes; an index is built for strings of up to " +
                                                 std::to_string(kCollateMaxBytes) + " bytes");
        co->max_bytes = (int)lw[0];
        co->gshift = std::min(3, __builtin_ctzll((unsigned long long)lw[1] | 8ull));
        // 2. order words, 3. the sort: least significant word first, each word a stable sort on top of the order so far
        const int nwords = (co->max_bytes + 7) / 8;
        BufP words = dev_alloc(c, sizeof(uint64_t) * (size_t)nwords * (size_t)d);
        HIP_CHECK(launch_collate_words(heap, n, (const int64_t *)off->p, d, nwords, (uint64_t *)words->p, s));
        mark("Words");
        if (d > 1)
            for (int j = nwords - 1; j >= 0; j--) order_sort_key(c, s, (const int64_t *)words->p + (int64_t)j * d, 0, d, stw, perm);
        mark("Sort");
        // 4. dense ranks: head flags, one scan
        ranks = dev_alloc(c, sizeof(int64_t) * (size_t)(d + 1));
        HIP_CHECK(launch_collate_heads((const uint64_t *)words->p, perm ? (const int64_t *)perm->p : nullptr, d, nwords, (int64_t *)ranks->p, s));
        BufP sums = dev_alloc(c, sizeof(int64_t) * (size_t)(prefix_sum_blocks(d + 1) + 1));
        HIP_CHECK(launch_prefix_sum((int64_t *)ranks->p, d + 1, (int64_t *)sums->p, s));
        c->fetch_to_host((const int64_t *)ranks->p + d, 1, &co->distinct, s);
        if (co->distinct < 1 || co->distinct > d) throw Error(VDL_ERR_DEVICE, "internal: collation of '" + name + "' ranked " + std::to_string(co->distinct) + " distinct strings of " + std::to_string(d));
        mark("Ranks");
    }
    co->table = dev_alloc(c, sizeof(int32_t) * (size_t)collate_table_slots(n, co->gshift));
    HIP_CHECK(launch_collate_table(heap, n, co->gshift, off ? (const int64_t *)off->p : nullptr, perm ? (const int64_t *)perm->p : nullptr,
                                   ranks ? (const int64_t *)ranks->p : nullptr, d, (int32_t *)co->table->p, s));
    mark("Table");
    HIP_CHECK(hipStreamSynchronize(s));
    for (size_t k = 1; steps && k < marks.size(); k++) {
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, marks[k - 1].second, marks[k].second));
        steps->push_back({std::string("timeInMicrosecondsForCollation") + marks[k].first + "_" + name, (double)ms * 1e3});
    }
    return co;
}

Column &heap_column(vdl_ctx *c, const std::string &heap, const std::string &who) {
    auto it = c->cols.find(heap);
    if (it == c->cols.end()) throw Error(VDL_ERR_ARG, who + ": heap column '" + heap + "' is not registered");
    return it->second;
}

}  // namespace

std::shared_ptr<Collation> collation_ensure(vdl_ctx *c, const std::string &heap, vdl_plan *p, const std::string &who) {
    Column &col = heap_column(c, heap, who);
    if (col.collation) return col.collation;
    need_device(c);
    EventPair ev;
    if (p) {
        HIP_CHECK(hipEventCreate(&ev.a)); HIP_CHECK(hipEventCreate(&ev.b));
        HIP_CHECK(hipEventRecord(ev.a, c->stream));
    }
    std::vector<Timing> steps;
    col.collation = collation_build(c, heap, col, p && p->profiling ? &steps : nullptr);
    if (p) {
        HIP_CHECK(hipEventRecord(ev.b, c->stream));
        HIP_CHECK(hipEventSynchronize(ev.b));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, ev.a, ev.b));
        p->timings.push_back({"timeInMicrosecondsForCollation_" + heap, (double)ms * 1e3});
        for (const Timing &t : steps) p->timings.push_back(t);      // with profiling: "..CollationMark_<heap>", "..Starts_", "..Words_", "..Sort_", "..Ranks_", "..Table_"
    }
    return col.collation;
}

std::vector<BufP> order_text_ranks(vdl_ctx *c, vdl_plan *p, const std::vector<const int64_t *> &codes, int64_t m, hipStream_t s) {
    const size_t nk = p->order.nodes.size();
    std::vector<BufP> out(nk);
    if (m <= 0 || p->order.n_text() == 0) return out;
    BufP st = dev_alloc(c, sizeof(uint64_t) * 2 * nk);
    HIP_CHECK(hipMemsetAsync(st->p, 0, sizeof(uint64_t) * 2 * nk, s));
    EventPair ev;                                                       // with profiling: the translate launches alone, under a label of their own
    if (p->profiling) {
        HIP_CHECK(hipEventCreate(&ev.a)); HIP_CHECK(hipEventCreate(&ev.b));
        HIP_CHECK(hipEventRecord(ev.a, s));
    }
    for (size_t k = 0; k < nk; k++) {
        const std::string &heap = p->order.text[k];
        if (heap.empty()) continue;
        const Column &col = heap_column(c, heap, "order key '" + p->prog.at(p->order.nodes[k]).field + "'");
        if (!col.collation) throw Error(VDL_ERR_DEVICE, "internal: heap '" + heap + "' has no collation index at the order step");
        const Collation &co = *col.collation;
        out[k] = dev_alloc(c, sizeof(int64_t) * (size_t)m);
        HIP_CHECK(launch_order_textkey(codes[k], m, (const int8_t *)col.dev, co.heap_n, co.table ? (const int32_t *)co.table->p : nullptr, co.gshift,
                                       (int64_t *)out[k]->p, (uint64_t *)st->p + 2 * k, s));
    }
    if (ev.b) HIP_CHECK(hipEventRecord(ev.b, s));
    std::vector<int64_t> verdict(2 * nk);
    c->fetch_to_host(st->p, 2 * nk, verdict.data(), s);
    if (ev.b) {
        float ms = 0;
        HIP_CHECK(hipEventSynchronize(ev.b));
        HIP_CHECK(hipEventElapsedTime(&ms, ev.a, ev.b));
        p->timings.push_back({"timeInMicrosecondsForOrderTextKeys", (double)ms * 1e3});
    }
    for (size_t k = 0; k < nk; k++) {
        if (verdict[2 * k] == 0) continue;
        const int64_t first = (int64_t)~(uint64_t)verdict[2 * k + 1];
        throw Error(VDL_ERR_SHAPE, "order key '" + p->prog.at(p->order.nodes[k]).field + "' is text over heap '" + p->order.text[k] + "', but " + std::to_string(verdict[2 * k]) +
                                       " of its " + std::to_string(m) + " rows hold a code that names no string of that heap (negative, at or past its " +
                                       std::to_string(heap_column(c, p->order.text[k], "order").n) + " bytes, or inside a string); the first is row " + std::to_string(first));
    }
    return out;
}

}  // namespace eng
}  // namespace vdl

using namespace vdl;
using namespace vdl::eng;

int vdl_build_collation(vdl_ctx *c, const char *heap_column) {
    if (!c || !heap_column) return VDL_ERR_ARG;
    return guard(c, [&] {
        need_device(c);
        if (!c->cols.count(heap_column)) throw Error(VDL_ERR_COLUMN, std::string("no column '") + heap_column + "'");
        collation_ensure(c, heap_column, nullptr, "vdl_build_collation");
    });
}

int vdl_collation_info(const vdl_ctx *c, const char *heap_column, int *present, int64_t *strings, int64_t *distinct, int *max_bytes) {
    if (!c || !heap_column) return VDL_ERR_ARG;
    auto it = c->cols.find(heap_column);
    if (it == c->cols.end()) return VDL_ERR_COLUMN;
    const Collation *co = it->second.collation.get();
    if (present) *present = co ? 1 : 0;
    if (strings) *strings = co ? co->strings : 0;
    if (distinct) *distinct = co ? co->distinct : 0;
    if (max_bytes) *max_bytes = co ? co->max_bytes : 0;
    return VDL_OK;
}

int vdl_collate_device(vdl_ctx *c, const char *heap_column, const int64_t *codes, int64_t m, int64_t *ranks_out, int64_t *n_bad, int64_t *first_bad) {
    if (!c || !heap_column || m < 0 || (m > 0 && (!codes || !ranks_out))) return VDL_ERR_ARG;
    return guard(c, [&] {
        need_device(c);
        if (!c->cols.count(heap_column)) throw Error(VDL_ERR_COLUMN, std::string("no column '") + heap_column + "'");
        const std::shared_ptr<Collation> co = collation_ensure(c, heap_column, nullptr, "vdl_collate_device");
        int64_t verdict[2] = {0, -1};
        if (m > 0) {
            hipStream_t s = c->stream;
            BufP in = dev_alloc(c, sizeof(int64_t) * (size_t)m), out = dev_alloc(c, sizeof(int64_t) * (size_t)m), st = dev_alloc(c, sizeof(uint64_t) * 2);
            HIP_CHECK(hipMemcpyAsync(in->p, codes, sizeof(int64_t) * (size_t)m, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipMemsetAsync(st->p, 0, sizeof(uint64_t) * 2, s));
            HIP_CHECK(launch_order_textkey((const int64_t *)in->p, m, (const int8_t *)c->cols[heap_column].dev, co->heap_n, co->table ? (const int32_t *)co->table->p : nullptr,
                                           co->gshift, (int64_t *)out->p, (uint64_t *)st->p, s));
            HIP_CHECK(hipMemcpyAsync(ranks_out, out->p, sizeof(int64_t) * (size_t)m, hipMemcpyDeviceToHost, s));
            int64_t w[2];
            c->fetch_to_host(st->p, 2, w, s);
            HIP_CHECK(hipStreamSynchronize(s));
            verdict[0] = w[0];
            verdict[1] = w[0] ? (int64_t)~(uint64_t)w[1] : -1;
        }
        if (n_bad) *n_bad = verdict[0];
        if (first_bad) *first_bad = verdict[1];
    });
}

// The definition of the ranks, device-free: strings cut at their NUL or the heap's end, compared as unsigned bytes with a prefix before
// its extensions, equal strings sharing a rank.
int vdl_collate_host(const int8_t *heap, int64_t heap_n, const int64_t *codes, int64_t m, int64_t *ranks_out, int64_t *n_bad, int64_t *first_bad) {
    if (heap_n < 0 || m < 0 || (heap_n > 0 && !heap) || (m > 0 && (!codes || !ranks_out))) return VDL_ERR_ARG;
    try {
        const unsigned char *h = (const unsigned char *)heap;
        struct Str { int64_t at, len; };
        std::vector<Str> strs;
        for (int64_t i = 0; i < heap_n; i++) {
            if (h[i] == 0 || (i > 0 && h[i - 1] != 0)) continue;
            int64_t e = i;
            while (e < heap_n && h[e] != 0) e++;
            strs.push_back({i, e - i});
        }
        auto cmp = [&](const Str &a, const Str &b) {
            const int r = std::memcmp(h + a.at, h + b.at, (size_t)std::min(a.len, b.len));      // memcmp compares unsigned bytes
            return r != 0 ? r : a.len < b.len ? -1 : a.len > b.len ? 1 : 0;
        };
        std::sort(strs.begin(), strs.end(), [&](const Str &a, const Str &b) { const int r = cmp(a, b); return r != 0 ? r < 0 : a.at < b.at; });
        std::vector<int64_t> rank_at((size_t)heap_n, -1);
        int64_t rank = 0;
        for (size_t k = 0; k < strs.size(); k++) {
            if (k == 0 || cmp(strs[k - 1], strs[k]) != 0) rank++;
            rank_at[(size_t)strs[k].at] = rank;
        }
        int64_t bad = 0, first = -1;
        for (int64_t i = 0; i < m; i++) {
            const int64_t code = codes[i];
            int64_t r = -1;
            if (code >= 0 && code < heap_n) r = h[code] == 0 ? 0 : rank_at[(size_t)code];
            ranks_out[i] = r;
            if (r < 0) { if (bad++ == 0) first = i; }
        }
        if (n_bad) *n_bad = bad;
        if (first_bad) *first_bad = first;
    } catch (const std::bad_alloc &) { return VDL_ERR_NOMEM; }
    return VDL_OK;
}
