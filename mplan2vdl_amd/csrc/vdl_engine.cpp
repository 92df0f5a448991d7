// vdl_engine.cpp -- context, column catalog, HBM pool, plan execution and the C ABI (include/vdl.h).
//
// Two execution strategies, both HIP-only (there is no CPU fallback anywhere in this library):
//   * fused   : programs of the "filter -> gather -> global fold" shape run as one read-once scan
//               per table (vdl_fuse.cpp decides, k_scan executes);
//   * general : any other program runs statement by statement with one kernel per operator;
//               RangeV/RangeC, Project, Shuffle and identity Gathers never touch memory.
// This file runs things; how a planned scan and the catalog's columns become kernel arguments is vdl_bind.cpp.
#include <atomic>
#include <chrono>

#include "vdl_genexec.h"
#include "vdl_specialise.h"

namespace {

// the descriptor `d` on the device under `role` (vdl_plan::desc_slots): uploaded when none of the role's copies already holds these
// bytes.  A role keeps up to three copies, the least recently used one is overwritten: the fused front's take descriptor names the
// output buffers, which alternate between two sets of addresses from run to run (the last run's results are still the plan's when
// the next run allocates), and with one copy per role every query paid a 5 us upload in the stream.
static const MScanDesc *desc_on_device(vdl_ctx *c, vdl_plan *p, const std::string &role, const MScanDesc &d) {
    constexpr int kCopies = 3;
    vdl_plan::DescSlot *hit = nullptr, *oldest = nullptr;
    for (int k = 0; k < kCopies; k++) {
        vdl_plan::DescSlot &sl = p->desc_slots[role + "#" + std::to_string(k)];
        if (sl.shadow.size() == sizeof(MScanDesc) && std::memcmp(sl.shadow.data(), &d, sizeof(MScanDesc)) == 0) { hit = &sl; break; }
        if (!oldest || sl.used < oldest->used) oldest = &sl;
    }
    uint64_t &clock = p->desc_clock;
    if (hit) { hit->used = ++clock; return (const MScanDesc *)hit->dev->p; }
    vdl_plan::DescSlot &sl = *oldest;
    if (!sl.dev) sl.dev = dev_alloc(c, sizeof(MScanDesc));
    // the shadow is the SOURCE of the copy: it stays put until the next upload, the caller's `d` may be a local
    sl.shadow.assign((const unsigned char *)&d, (const unsigned char *)&d + sizeof(MScanDesc));
    sl.used = ++clock;
    HIP_CHECK(hipMemcpyAsync(sl.dev->p, sl.shadow.data(), sizeof(MScanDesc), hipMemcpyHostToDevice, c->stream));
    return (const MScanDesc *)sl.dev->p;
}

// ------------------------------------------------------------------------------------------------
// fused execution
// ------------------------------------------------------------------------------------------------
struct NeedGeneralPath : Error {          // a fused assumption did not hold for this data: rerun unfused
    explicit NeedGeneralPath(const std::string &m) : Error(VDL_ERR_UNSUPPORTED, m) {}
};

int64_t plan_words(const vdl_plan *p, std::vector<int32_t> *ops, bool *shardable) {
    int64_t off = 0;
    if (shardable) *shardable = true;
    for (const ScanPlan &sp : p->fused.scans) {
        if (ops) {
            ops->push_back(VDL_REDUCE_SUM);
            for (const ScanAgg &ag : sp.aggs) ops->push_back(ag.kind == AGG_SUM ? VDL_REDUCE_SUM : ag.kind == AGG_MIN ? VDL_REDUCE_MIN : VDL_REDUCE_MAX);
        }
        off += (int64_t)sp.aggs.size() + 1;
    }
    for (const GroupScanPlan &gp : p->fused.gscans) {
        for (int64_t b = 0; b < gp.pcount; b++) {
            if (ops) ops->push_back(VDL_REDUCE_SUM);
            for (const ScanAgg &ag : gp.aggs) {
                if (ops) ops->push_back(ag.kind == AGG_SUM ? VDL_REDUCE_SUM : ag.kind == AGG_MAX ? VDL_REDUCE_MAX
                                        : ag.kind == AGG_FIRST ? VDL_REDUCE_FIRST : VDL_REDUCE_MIN);
            }
        }
        if (ops) ops->push_back(VDL_REDUCE_SUM);                              // out-of-domain key count
        off += gp.pcount * ((int64_t)gp.aggs.size() + 1) + 1;
    }
    // a semi-join set is built from ALL selected rows of its source table: a rank that holds a shard of either table would test
    // (or build) a partial set
    if (shardable) for (const PreludeItem &it : p->fused.prelude) if (it.kind == PreludeItem::SEMI_BITMAP) *shardable = false;
    return off;
}

// the precompiled multi-aggregate kernel's name, ",img" where some columns are read from their images (as the specialised kernels' names: vdl_specialise.cpp)
static std::string mscan_label(const ScanLaunch &cfg, const MScanCols &cols) {
    std::string n = mscan_kernel_name(cfg);
    if (cols.image && !n.empty() && n.back() == '>') n.insert(n.size() - 1, ",img");
    if (cols.limage && !n.empty() && n.back() == '>') n.insert(n.size() - 1, ",limg");      // (a lookup reads its target's image)
    return n;
}
// ... and ",wide" where the wide-sums build of it runs (vdl_mscan_wide.hip)
static std::string mscan_label(const ScanLaunch &cfg, const MScanCols &cols, const MScanDesc &d) {
    std::string n = mscan_label(cfg, cols);
    if (d.wide && !n.empty() && n.back() == '>') n.insert(n.size() - 1, ",wide");
    return n;
}
// blocks a specialised scan may be launched with, whatever rows-per-lane the tuner settles on: the partials area is sized for it
static int max_scan_grid(const vdl_ctx *c, const vdl_plan *p, int chosen) { return p->use_jit ? std::max(chosen, c->num_cus * 8) : chosen; }


void bind_fused(vdl_ctx *c, vdl_plan *p) {
    const FusedPlan &F = p->fused;
    const size_t ns = F.scans.size(), ng = F.gscans.size();
    p->sargs.assign(ns, ScanArgs{});
    p->scfg.assign(ns, ScanLaunch{});
    p->block_partials.assign(ns, nullptr);
    p->word_offset.assign(ns, 0);
    p->mcols.assign(ns + ng, MScanCols{});
    p->mdesc.assign(ns + ng, MScanDesc{});
    p->mcfg.assign(ns + ng, ScanLaunch{});
    p->mparts.assign(ns + ng, nullptr);
    p->mdev.resize(ns + ng);
    p->mjit.assign(ns + ng, nullptr);
    p->mjit_form.assign(ns + ng, ScanForm{});
    p->kscan.assign(ns + ng, 0);
    p->jit_note.clear();
    p->wide_note.clear();
    p->jit_builds.clear();
    for (auto it = p->roles.begin(); it != p->roles.end();) it = it->first.compare(0, 4, "scan") == 0 ? p->roles.erase(it) : std::next(it);
    p->jit_tuned = false;
    p->gword_offset.assign(ng, 0);
    p->reduce_ops.clear();
    bool shardable = true;
    p->n_words = plan_words(p, &p->reduce_ops, &shardable);
    int64_t off = 0;
    p->scan_rows = 0; p->scan_bytes = 0; p->dominant = -1;
    p->dominant_kernel = "none";
    for (size_t s = 0; s < ns; s++) {
        const ScanPlan &sp = F.scans[s];
        int64_t bpr = 0, n = 0;
        std::string kname;
        const bool eligible = use_kscan(sp);
        // (wide sums: k_scan has no wide build -- a single-sum scan runs on k_mscan's)
        p->kscan[s] = eligible && !(p->use_jit && !sp.never) && !p->wide;    // specialising: the single-aggregate scan runs through the general body too
        if (eligible) {                                       // (bound either way: the tuner compares the two)
            ScanArgs &a = p->sargs[s];
            n = bind_kscan(c, sp, a, &bpr);
            p->scfg[s] = scan_launch_config(a, c->num_cus);
            if (p->scfg[s].variant < 0) throw Error(VDL_ERR_UNSUPPORTED, "no scan kernel variant for this shape");
            p->block_partials[s] = dev_alloc(c, sizeof(int64_t) * (size_t)p->scfg[s].grid * 2);
            a.block_partials = (int64_t *)p->block_partials[s]->p;
            kname = std::string(scan_kernel_name(p->scfg[s])) + "_grid" + std::to_string(p->scfg[s].grid);
        }
        if (!p->kscan[s]) {
            n = bind_scan(c, p, s, p->mcols[s], p->mdesc[s], &bpr, p->row_offset);
            p->mdesc[s].wide = p->wide ? 1 : 0;
            note_roles(p, "scan" + std::to_string(s), sp.cols, p->mcols[s]);
            p->mcfg[s] = mscan_launch_config(p->mcols[s], p->mdesc[s], false, c->num_cus);
            if (p->mcfg[s].variant < 0) throw Error(VDL_ERR_UNSUPPORTED, "no multi-aggregate scan kernel variant for this shape");
            std::string jname;
            const bool spec = p->use_jit && !sp.never && specialise_scan(c, p, s, false, &jname);
            if (eligible && !spec && !p->wide) { p->kscan[s] = 1; }       // it did not build: the tuned single-aggregate kernel after all
            p->mparts[s] = dev_alloc(c, sizeof(int64_t) * (size_t)max_scan_grid(c, p, p->mcfg[s].grid) * (size_t)mscan_partial_words(p->mdesc[s], false));
            p->mdesc[s].block_partials = (int64_t *)p->mparts[s]->p;
            if (!p->mdev[s]) p->mdev[s] = dev_alloc(c, sizeof(MScanDesc));
            if (!p->kscan[s]) kname = (spec ? jname : mscan_label(p->mcfg[s], p->mcols[s], p->mdesc[s])) + "_grid" + std::to_string(p->mcfg[s].grid);
            if (p->wide) p->wide_note += std::string(p->wide_note.empty() ? "wide: " : "; ") + (spec ? jname : mscan_label(p->mcfg[s], p->mcols[s], p->mdesc[s])) + " global, " +
                                         std::to_string(mscan_sums(p->mdesc[s])) + " sums";
        }
        p->word_offset[s] = off;
        off += (int64_t)sp.aggs.size() + 1;
        if (!sp.never && n * bpr > p->scan_bytes) { p->scan_bytes = n * bpr; p->scan_rows = n; p->dominant = (int)s; p->dominant_kernel = kname; }
    }
    for (size_t g = 0; g < ng; g++) {
        const GroupScanPlan &gp = F.gscans[g];
        const size_t m = ns + g;
        int64_t bpr = 0;
        const int64_t n = bind_scan(c, p, m, p->mcols[m], p->mdesc[m], &bpr, p->row_offset);
        note_roles(p, "scan" + std::to_string(m), gp.cols, p->mcols[m]);
        MScanDesc &d = p->mdesc[m];
        d.wide = p->wide ? 1 : 0;
        p->mcfg[m] = mscan_launch_config(p->mcols[m], d, true, c->num_cus);
        if (p->mcfg[m].variant < 0) throw Error(VDL_ERR_UNSUPPORTED, "no grouped-scan kernel variant for this shape");
        // (wide sums: the table holds one more word per SUM aggregate and bucket; one replica of it has to fit what a block gets)
        if (d.wide && mscan_lds_bytes(d, true) > (size_t)kGroupLdsWords * sizeof(int64_t))
            throw Error(VDL_ERR_UNSUPPORTED, "wide sums: the group table of scan " + std::to_string(m) + ", " + std::to_string(d.pcount) + " buckets x (1 + " + std::to_string(d.nagg) +
                                             " aggregates + " + std::to_string(mscan_sums(d)) + " high words), leaves no room in LDS for one replica (" +
                                             std::to_string(mscan_lds_bytes(d, true)) + " of " + std::to_string((size_t)kGroupLdsWords * sizeof(int64_t)) + " bytes)");
        std::string jname;
        const bool spec = p->use_jit && !gp.never && specialise_scan(c, p, m, true, &jname);
        const int64_t words = d.pcount * (d.nagg + 1) + 1;
        p->mparts[m] = dev_alloc(c, sizeof(int64_t) * (size_t)max_scan_grid(c, p, p->mcfg[m].grid) * (size_t)mscan_partial_words(d, true));
        d.block_partials = (int64_t *)p->mparts[m]->p;
        if (!p->mdev[m]) p->mdev[m] = dev_alloc(c, sizeof(MScanDesc));
        p->gword_offset[g] = off;
        off += words;
        if (!gp.never && n * bpr > p->scan_bytes) {
            p->scan_bytes = n * bpr; p->scan_rows = n; p->dominant = (int)m;
            p->dominant_kernel = (spec ? jname : mscan_label(p->mcfg[m], p->mcols[m], d)) + "_grid" + std::to_string(p->mcfg[m].grid) + "_rep" + std::to_string(d.replicas);
        }
        if (p->wide) p->wide_note += std::string(p->wide_note.empty() ? "wide: " : "; ") + (spec ? jname : mscan_label(p->mcfg[m], p->mcols[m], d)) + " grouped, " +
                                     std::to_string(mscan_sums(d)) + " sums";
    }
    p->bound = true;
}

// One specialised pass of the projection scan: its translation unit, its entry point and what the note calls it
struct PassSource { std::string source, label; const char *entry; };
// the select pass (dimension and semi-join scans are the select pass with bitmap_only set)
// (rt: the plan's bounds at run time, vdl_plan_set_jit_bounds -- ",rtb" in the label)
static PassSource select_pass(const MScanCols &cols, const MScanDesc &d, bool rt) {
    jit::Shape sh;
    sh.nc = cols.ncol; sh.u = 4; sh.vec = project_select_vec(cols); sh.der = true; sh.rt_bounds = rt;
    return {jit::scan_source(jit::SELECT, mscan_args(cols), d, sh),
            std::string(jit::entry_name(jit::SELECT)) + "<" + std::to_string(sh.nc) + (cols.image ? ",img" : "") + (cols.limage ? ",limg" : "") + (cols.steps ? ",stp" : "") + (rt ? ",rtb" : "") + ">", jit::entry_name(jit::SELECT)};
}
// the one-pass front: two descriptors in one kernel (jit::front_source)
static PassSource one_pass_front(const MScanCols &scols, const MScanDesc &sd, const MScanCols &tcols, const MScanDesc &td, bool rt) {
    jit::Shape sh;
    sh.nc = scols.ncol; sh.u = 4; sh.vec = project_select_vec(scols); sh.der = true; sh.rt_bounds = rt;
    return {jit::front_source(mscan_args(scols), sd, mscan_args(tcols), td, sh, tcols.ncol),
            std::string(jit::entry_name(jit::FRONT)) + "<" + std::to_string(sh.nc) + "," + std::to_string(tcols.ncol) + ((scols.image | tcols.image) ? ",img" : "") + ((scols.limage | tcols.limage) ? ",limg" : "") + ((scols.steps | tcols.steps) ? ",stp" : "") + (rt ? ",rtb" : "") + ">",
            jit::entry_name(jit::FRONT)};
}
// Compiles the pass and writes its line of the note: "role: entry<shape[,img]>, N B of code; ".  A run loads the kernel and falls back
// to the precompiled one where it did not build ("role: not specialised (why); ", nullptr); vdl_plan_jit_check (`check`) loads
// nothing and throws
// (said: what was appended to the note, for a later rebuild of the role to take out again)
static std::shared_ptr<jit::Kernel> build_pass(vdl_ctx *c, vdl_plan *p, const std::string &role, const PassSource &ps, bool check, std::string *said = nullptr) {
    std::vector<char> code;
    std::string why;
    std::shared_ptr<jit::Kernel> k;
    jit::Origin from = jit::COMPILED;
    const bool built = jit::compile(ps.source, c->arch, code, why, &from);
    if (check && !built) throw Error(VDL_ERR_UNSUPPORTED, role + " does not build: " + why.substr(0, 2000));
    if (built && !check) k = jit::load(code, why, ps.entry);
    std::string line = k || check ? role + ": " + ps.label + ", " + std::to_string(code.size()) + " B of code; " : role + ": not specialised (" + why.substr(0, 400) + "); ";
    if (built && !check) { count_build(p, role, from); line += builds_text(p, role); }
    p->jit_note += line;
    if (said) *said = line;
    return k;
}
// The projection scan's passes specialised for this plan (vdl_plan_set_jit): built at the first run after a catalog change,
// kept by role ("front", "dim<k>", "semi<k>"); nullptr = the precompiled kernel (not asked for, or it did not build: the note says).
// (`source` is only called when the pass is built)
template <typename MakeSource>
static hipFunction_t front_kernel(vdl_ctx *c, vdl_plan *p, const std::string &role, MakeSource &&source) {
    if (!p->use_jit) return nullptr;
    vdl_plan::FrontKernel &fk = p->front_jit[role];
    if (fk.version == c->binding_version()) return fk.k ? fk.k->fn : nullptr;
    if (!fk.said.empty()) {   // a rebuild after a catalog change: what the role said last time (its line and its builds) leaves the note
        const size_t at = p->jit_note.find(fk.said);
        if (at != std::string::npos) p->jit_note.erase(at, fk.said.size());
        fk.said.clear();
        p->jit_builds.erase(role);
    }
    fk.version = c->binding_version();
    fk.k = nullptr;
    fk.k = build_pass(c, p, role, source(), false, &fk.said);
    return fk.k ? fk.k->fn : nullptr;
}

// Dimension-side work of scans with derived columns (FusedPlan::prelude): the per-operator executor runs the statements
// that hold the dimension selections (filters on the dimension table, joins of dimensions with further dimensions) and
// their validity bitmaps become the lookup tables of the fact scan; LIKE patterns are evaluated once per heap offset.
// Part of the query: runs on every execution.  `wanted[k]`: item k is referred to by a scan that is about to run.
// open (a join batch, batch_open_items): [k] = the dimension bitmap k is not built -- no table, every row of its table selected
// (g_prelude_items: prelude tables built in this process so far -- LIKE tables, dimension bitmaps by scan or by witness, semi-join sets;
// vdl_prelude_counters: what shows that a join batch builds its tables once and K plans alone K times)
static std::atomic<int64_t> g_prelude_items{0};
void run_prelude_items(vdl_ctx *c, vdl_plan *p, const std::vector<char> &asked, const std::vector<char> *open = nullptr) {
    const FusedPlan &F = p->fused;
    p->prelude_buf.assign(F.prelude.size(), nullptr);
    p->prelude_n.assign(F.prelude.size(), 0);
    p->prelude_rows.assign(F.prelude.size(), 0);
    std::vector<char> wanted(asked);
    for (size_t k = F.prelude.size(); k-- > 0;)                 // what a wanted dimension scan looks up itself (earlier items)
        if (wanted[k] && F.prelude[k].scan)
            for (const ScanColumn &sc : F.prelude[k].cols) if (sc.prelude >= 0) wanted[(size_t)sc.prelude] = 1;
    const bool scans = !getenv("VDL_NO_DIM_SCAN");
    // (an open bitmap: no words -- a lookup without a table selects every row -- over the rows of its table)
    for (size_t k = 0; open && k < F.prelude.size(); k++)
        if (wanted[k] && (*open)[k]) p->prelude_n[k] = find_col(c, F.prelude[k].cols[0].name).n;
    for (size_t k = 0; k < F.prelude.size(); k++) {
        const PreludeItem &it = F.prelude[k];
        if (!wanted[k] || it.kind != PreludeItem::LIKE_LUT) continue;
        const Column &heap = find_col(c, it.heap);
        Src offs; offs.kind = SRC_RANGE; offs.from = 0; offs.step = 1;
        Src hs; hs.p = heap.dev; hs.kind = heap.width == 8 ? SRC_I64 : heap.width == 4 ? SRC_I32 : heap.width == 2 ? SRC_I16 : SRC_I8;
        LikePattern pat{};
        pat.len = (int)it.pattern.size();
        memcpy(pat.p, it.pattern.data(), it.pattern.size());
        p->prelude_buf[k] = dev_alloc(c, sizeof(int64_t) * (size_t)std::max<int64_t>(heap.n, 1));
        p->prelude_n[k] = heap.n;
        HIP_CHECK(launch_like(offs, nullptr, heap.n, hs, nullptr, heap.n, pat, (int64_t *)p->prelude_buf[k]->p, c->stream));
        g_prelude_items++;
    }
    std::vector<int> witnesses;
    for (size_t k = 0; k < F.prelude.size(); k++)
        if (wanted[k] && F.prelude[k].kind == PreludeItem::DIM_BITMAP && !(scans && F.prelude[k].scan) && !(open && (*open)[k])) witnesses.push_back(F.prelude[k].witness);
    if (!witnesses.empty()) {
        GenExec g(c, p);
        g.run_nodes(witnesses, nullptr);
        for (size_t k = 0; k < F.prelude.size(); k++) {
            if (!wanted[k] || F.prelude[k].kind != PreludeItem::DIM_BITMAP || (scans && F.prelude[k].scan) || (open && (*open)[k])) continue;
            const DVec &v = g.vec[(size_t)F.prelude[k].witness];
            p->prelude_n[k] = v.n;
            g_prelude_items++;
            if (v.kind == DVec::SPARSE) p->prelude_buf[k] = g.bitmap_of(v.sel);
            else p->prelude_buf[k] = g.densify(v).valid;                  // null: every dimension row holds a value
        }
        HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    // dimension scans, in order: an item only looks up earlier ones
    std::vector<BufP> descs;
    // (host copies of the descriptors stay alive in the plan until its next run: the copies to the device are asynchronous)
    std::vector<std::shared_ptr<MScanDesc>> &host_descs = p->host_descs;
    host_descs.clear();
    for (size_t k = 0; k < F.prelude.size(); k++) {
        const PreludeItem &it = F.prelude[k];
        const bool semi = it.kind == PreludeItem::SEMI_BITMAP;
        if (!wanted[k] || !it.scan || !(semi || (scans && it.kind == PreludeItem::DIM_BITMAP))) continue;
        if (open && (*open)[k]) continue;
        MScanCols cols;
        host_descs.push_back(std::make_shared<MScanDesc>());
        MScanDesc *d = host_descs.back().get();
        g_prelude_items++;
        const int64_t n = bind_prelude_scan(c, p, k, cols, *d);
        patch_prelude(p, it.cols, cols, *d);
        if (semi) {
            // the set of rows of another table that a selected row of this one points at: one scan, atomic ORs
            const int64_t nbits = find_col(c, it.bits_of).n;
            if (it.modulus > 0 && nbits > it.modulus)
                throw NeedGeneralPath("the semi-join's positions are taken mod " + std::to_string(it.modulus) + " but the table they index has " + std::to_string(nbits) + " rows");
            const size_t words = (size_t)std::max<int64_t>((nbits + 63) >> 6, 1);
            p->prelude_buf[k] = dev_alloc(c, sizeof(uint64_t) * words);
            p->prelude_n[k] = nbits;
            HIP_CHECK(hipMemsetAsync(p->prelude_buf[k]->p, 0, sizeof(uint64_t) * words, c->stream));
            p->prelude_rows[k] = std::max<int64_t>(n, 0);
            if (it.never || n <= 0) continue;
            // the Scatter this set stands for writes into a vector as long as ITS table (the fold operand, Vlite.hs:1212-1222):
            // positions at or beyond that length are dropped like any out-of-range Scatter position, also when the indexed
            // table is the longer one
            // (sharded: n is this rank's share of the table; the merge clips at the global length: semi_unclamped)
            d->dn[it.index_col] = p->semi_unclamped ? nbits : std::min(nbits, n);
            p->prelude_rows[k] = n;
            d->out_ptr[0] = (int64_t *)p->prelude_buf[k]->p;
            HIP_CHECK(launch_project_select(cols, desc_on_device(c, p, "semi" + std::to_string(k), *d), c->num_cus, c->stream,
                                            front_kernel(c, p, "semi" + std::to_string(k), [&] { return select_pass(cols, *d, p->jit_rt_bounds); })));
            continue;
        }
        const size_t words = (size_t)std::max<int64_t>((n + 63) >> 6, 1);
        p->prelude_buf[k] = dev_alloc(c, sizeof(uint64_t) * words);
        p->prelude_n[k] = n;
        if (it.never || n <= 0) { HIP_CHECK(hipMemsetAsync(p->prelude_buf[k]->p, 0, sizeof(uint64_t) * words, c->stream)); continue; }
        d->out_ptr[0] = (int64_t *)p->prelude_buf[k]->p;           // bitmap only: no positions, no counts
        HIP_CHECK(launch_project_select(cols, desc_on_device(c, p, "dim" + std::to_string(k), *d), c->num_cus, c->stream,
                                        front_kernel(c, p, "dim" + std::to_string(k), [&] { return select_pass(cols, *d, p->jit_rt_bounds); })));
    }
}
void run_prelude(vdl_ctx *c, vdl_plan *p) {
    const FusedPlan &F = p->fused;
    if (F.prelude.empty()) return;
    std::vector<char> wanted(F.prelude.size(), 0);
    const size_t nscans = F.scans.size() + F.gscans.size();
    for (size_t s = 0; s < nscans; s++)
        for (const ScanColumn &sc : scan_columns(p, s))
            if (sc.prelude >= 0) wanted[(size_t)sc.prelude] = 1;
    run_prelude_items(c, p, wanted);
    if (p->after_prelude) p->after_prelude(c, p);
    for (size_t s = 0; s < nscans; s++) patch_prelude(p, scan_columns(p, s), p->mcols[s], p->mdesc[s]);
}

void run_fused_local(vdl_ctx *c, vdl_plan *p, int64_t *dev_words, bool single_rank) {
    const char *tune_a = getenv("VDL_SCAN_TUNE"), *tune_b = getenv("VDL_GROUP_TUNE");
    if (!p->bound || p->bound_version != c->binding_version() || tune_a || tune_b) {   // tuning sweeps re-bind every run
        bind_fused(c, p);
        p->bound_version = c->binding_version();
    }
    // wide sums: the high words of the partial words, laid out as dev_words is (the finish step of every scan writes both)
    int64_t *hi_words = nullptr;
    if (p->wide) {
        if (!p->wide_hi || p->wide_hi_cap < p->n_words) { p->wide_hi = dev_alloc(c, sizeof(int64_t) * (size_t)std::max<int64_t>(p->n_words, 1)); p->wide_hi_cap = p->n_words; }
        // (a sharded run: straight into its slot's send buffer -- wide_hi is one buffer per plan, and the next query's local phase runs
        // while this query's gather is still queued; the tuner's candidates keep using wide_hi)
        hi_words = p->wide_hi_out ? p->wide_hi_out : (int64_t *)p->wide_hi->p;
    }
    run_prelude(c, p);
    if (p->use_jit && p->jit_tune && !p->jit_tuned) {
        p->jit_tuned = true;
        for (size_t s = 0; s < p->mcols.size(); s++)              // (the lookup tables of this run are in place)
            if (p->mjit[s]) patch_prelude(p, scan_columns(p, s), p->mcols[s], p->mdesc[s]);
        tune_specialised(c, p, dev_words);
    }
    const int ei = (int)(p->run_seq++ % (unsigned)vdl_plan::kEvRing);
    if (p->profiling && !p->ev0[ei]) { HIP_CHECK(hipEventCreate(&p->ev0[ei])); HIP_CHECK(hipEventCreate(&p->ev1[ei])); }
    p->ev_pending[ei] = false;
    p->ev_bound[ei] = false;
    p->ev_seq[ei] = p->run_seq;
    p->last_ev = ei;
    p->ev_buf[ei] = dev_words;
    const size_t ns = p->fused.scans.size(), ng = p->fused.gscans.size();
    for (size_t s = 0; s < ns + ng; s++) {
        const bool grouped = s >= ns;
        const bool never = grouped ? p->fused.gscans[s - ns].never : p->fused.scans[s].never;
        int64_t *out = dev_words + (grouped ? p->gword_offset[s - ns] : p->word_offset[s]);
        const bool kscan = !grouped && p->kscan[s];
        const int64_t n = kscan ? p->sargs[s].n : p->mcols[s].n;
        const bool timed = p->profiling && (int)s == p->dominant && !never && n > 0;
        if (kscan) {
            const ScanArgs &a = p->sargs[s];
            int nblocks = 0;
            if (!never && n > 0) {
                if (timed) HIP_CHECK(hipEventRecord(p->ev0[ei], c->stream));
                HIP_CHECK(launch_scan(a, p->scfg[s], c->stream));
                if (timed) { HIP_CHECK(hipEventRecord(p->ev1[ei], c->stream)); p->ev_pending[ei] = true; }
                nblocks = p->scfg[s].grid;
            }
            HIP_CHECK(launch_scan_finish(a.block_partials, nblocks, a.nagg, nullptr, a, out, c->stream));
        } else {
            const MScanDesc *on_dev = desc_on_device(c, p, "scan" + std::to_string(s), p->mdesc[s]);
            // events bracket the scan together with its tiny finish kernel(s)
            if (timed) HIP_CHECK(hipEventRecord(p->ev0[ei], c->stream));
            HIP_CHECK(launch_mscan(p->mcols[s], p->mdesc[s], on_dev, p->mcfg[s], grouped, never, out,
                                   grouped && single_rank, c->stream, p->mjit[s] ? p->mjit[s]->fn : nullptr,
                                   hi_words ? hi_words + (grouped ? p->gword_offset[s - ns] : p->word_offset[s]) : nullptr));
            if (timed) { HIP_CHECK(hipEventRecord(p->ev1[ei], c->stream)); p->ev_pending[ei] = true; }
        }
    }
}

// Finalisation is split so that callers can pipeline queries: `begin` enqueues the copy of the
// (merged) partial words into a pinned host slot and records an event; `end` waits for that event
// only (not for younger work on the stream) and builds the outputs.
void finalize_begin(vdl_ctx *c, vdl_plan *p, const int64_t *dev_words, int slot) {
    if (!p->bound && !p->batch_words) throw Error(VDL_ERR_ARG, "vdl_finalize called before vdl_run_local");
    if (slot < 0 || slot > 1) throw Error(VDL_ERR_ARG, "finalisation slot must be 0 or 1");
    if (p->host_cap < p->n_words) {
        for (int k = 0; k < 2; k++) {
            if (p->host_words[k]) HIP_CHECK(hipHostFree(p->host_words[k]));
            HIP_CHECK(hipHostMalloc((void **)&p->host_words[k], sizeof(int64_t) * (size_t)std::max<int64_t>(p->n_words, 1), hipHostMallocDefault));
        }
        p->host_cap = p->n_words;
    }
    if (!p->slot_ev[slot]) HIP_CHECK(hipEventCreateWithFlags(&p->slot_ev[slot], hipEventDisableTiming));
    if (p->n_words) HIP_CHECK(hipMemcpyAsync(p->host_words[slot], dev_words, sizeof(int64_t) * (size_t)p->n_words, hipMemcpyDeviceToHost, c->stream));
    // wide sums: the high words travel beside the low ones into a pinned buffer of the slot's own -- a sharded wide run is pipelined
    // like any other, and hands over its MERGED high words (wide_hi_src); vdl_run's are where its scans left them
    const int64_t *hi_src = p->wide_hi_src ? p->wide_hi_src : p->wide_hi ? (const int64_t *)p->wide_hi->p : nullptr;
    p->slot_wide[slot] = p->wide && hi_src && p->n_words;
    if (p->slot_wide[slot]) {
        if (p->host_hi_cap < p->n_words) {
            for (int k = 0; k < 2; k++) {
                if (p->host_hi[k]) HIP_CHECK(hipHostFree(p->host_hi[k]));
                p->host_hi[k] = nullptr;
            }
            p->host_hi_cap = 0;
            for (int k = 0; k < 2; k++) HIP_CHECK(hipHostMalloc((void **)&p->host_hi[k], sizeof(int64_t) * (size_t)p->n_words, hipHostMallocDefault));
            p->host_hi_cap = p->n_words;
        }
        HIP_CHECK(hipMemcpyAsync(p->host_hi[slot], hi_src, sizeof(int64_t) * (size_t)p->n_words, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_CHECK(hipEventRecord(p->slot_ev[slot], c->stream));
    p->slot_pending[slot] = true;
    int ei = -1;
    for (int k = 0; k < vdl_plan::kEvRing; k++)      // the oldest run into this buffer whose timing nobody has claimed
        if (p->ev_pending[k] && !p->ev_bound[k] && p->ev_buf[k] == (const void *)dev_words && (ei < 0 || p->ev_seq[k] < p->ev_seq[ei])) ei = k;
    if (ei >= 0) p->ev_bound[ei] = true;
    p->slot_ev_idx[slot] = ei;
}

void finalize_end(vdl_ctx *c, vdl_plan *p, int slot) {
    if (slot < 0 || slot > 1 || !p->slot_pending[slot]) throw Error(VDL_ERR_ARG, "no finalisation pending in this slot");
    HIP_CHECK(hipEventSynchronize(p->slot_ev[slot]));
    p->slot_pending[slot] = false;
    const int64_t *wp = p->host_words[slot];
    std::vector<int64_t> w(wp, wp + p->n_words);
    (void)c;
    p->timings.clear();
    if (p->slot_ev_idx[slot] >= 0) {
        const int ei = p->slot_ev_idx[slot];
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, p->ev0[ei], p->ev1[ei]));
        p->scan_usec = (double)ms * 1e3;
        p->timings.push_back({"timeInMicrosecondsForFusedScan_" + p->dominant_kernel, p->scan_usec});
        p->ev_pending[ei] = false;
        p->slot_ev_idx[slot] = -1;
    }
    const size_t ns = p->fused.scans.size();
    for (size_t g = 0; g < p->fused.gscans.size(); g++) {
        const MScanDesc &a = p->mdesc[ns + g];
        const int64_t oob = w[(size_t)(p->gword_offset[g] + a.pcount * (a.nagg + 1))];
        if (oob > 0)
            throw NeedGeneralPath(std::to_string(oob) + " row(s) carry a group key outside the Partition pivots [" + std::to_string(a.pmin) + "," +
                                  std::to_string(a.pmin + a.pcount - 1) + "]");
    }
    p->outs.clear();
    // wide sums: every output from the exact 128-bit aggregate values (the low words are `w`, the high words came beside them); the
    // high word of a MIN, MAX or FIRST aggregate is its sign extension (a FIRST word became a column value after the finish step)
    const bool wide = p->wide && p->slot_wide[slot] && p->host_hi[slot] && p->host_hi_cap >= p->n_words;
    if (p->wide && !wide && p->n_words) throw Error(VDL_ERR_ARG, "internal: a wide-sums run without its high words");
    const std::vector<int64_t> wh(wide ? p->host_hi[slot] : nullptr, wide ? p->host_hi[slot] + p->n_words : nullptr);      // this slot's, as `w`
    auto wide_values = [&](const int64_t *lo, const int64_t *hi, const MScanDesc &a, std::vector<wide_t> &v) {
        v.resize((size_t)a.nagg + 1);
        v[0] = (wide_t)lo[0];
        for (int j = 0; j < a.nagg; j++) {
            const int64_t h = a.agg[j].kind == AGG_SUM ? hi[1 + j] : (lo[1 + j] >> 63);
            v[(size_t)j + 1] = (wide_t)(((unsigned __int128)(uint64_t)h << 64) | (uint64_t)lo[1 + j]);
        }
    };
    auto push_wide = [&](Output &o, wide_t x) {
        o.vals.push_back((int64_t)(uint64_t)(unsigned __int128)x);
        o.hi.push_back((int64_t)(uint64_t)((unsigned __int128)x >> 64));
    };
    std::vector<wide_t> wv;
    for (const FusedOutput &fo : p->fused.outputs) {
        Output o;
        o.node = fo.node;
        o.name = p->prog.at(fo.node).field;
        o.tmp = "tmp" + std::to_string(fo.node);
        o.has_hi = wide;
        if (wide && fo.gscan < 0) {
            const int64_t *sw = w.data() + p->word_offset[(size_t)fo.scan];
            if (sw[0] > 0) { wide_values(sw, wh.data() + p->word_offset[(size_t)fo.scan], p->mdesc[(size_t)fo.scan], wv); push_wide(o, eval_scalar_wide(*fo.value, wv.data() + 1)); }
        } else if (wide) {
            const MScanDesc &a = p->mdesc[ns + (size_t)fo.gscan];
            const int W = a.nagg + 1;
            const int64_t *tab = w.data() + p->gword_offset[(size_t)fo.gscan], *tabh = wh.data() + p->gword_offset[(size_t)fo.gscan];
            for (int64_t b = 0; b < a.pcount; b++)
                if (tab[b * W] > 0) { wide_values(tab + b * W, tabh + b * W, a, wv); push_wide(o, eval_scalar_wide(*fo.value, wv.data() + 1)); }
        } else
        if (fo.gscan < 0) {
            const int64_t *sw = w.data() + p->word_offset[(size_t)fo.scan];
            if (sw[0] > 0) o.vals.push_back(eval_scalar(*fo.value, sw + 1));   // no selected row -> the fold slot is EPS
        } else {
            // one value per non-empty bucket, ascending = the order of the runs of the sorted key
            const MScanDesc &a = p->mdesc[ns + (size_t)fo.gscan];
            const int W = a.nagg + 1;
            const int64_t *tab = w.data() + p->gword_offset[(size_t)fo.gscan];
            for (int64_t b = 0; b < a.pcount; b++)
                if (tab[b * W] > 0) o.vals.push_back(eval_scalar(*fo.value, tab + b * W + 1));
        }
        p->outs.push_back(std::move(o));
    }
}

}  // namespace

namespace vdl {
namespace eng {

// ---- the order step on the host ----------------------------------------------------------------------------------------------
int64_t order_resolve(const vdl_plan *p, std::vector<size_t> &keys) {
    int64_t m = p->outs.empty() ? 0 : (int64_t)p->outs[0].count();
    bool same = true;
    for (const Output &o : p->outs) same = same && (int64_t)o.count() == m;
    if (!same) {
        std::string all;
        for (const Output &o : p->outs) all += (all.empty() ? "" : ", ") + o.name + " (" + o.tmp + "): " + std::to_string(o.count());
        throw Error(VDL_ERR_SHAPE, "an order is set, but the outputs are not the columns of one result; their lengths: " + all);
    }
    keys.clear();
    for (int node : p->order.nodes) {
        size_t at = p->outs.size();
        for (size_t k = 0; k < p->outs.size(); k++) if (p->outs[k].node == node) { at = k; break; }
        if (at == p->outs.size()) throw Error(VDL_ERR_SHAPE, "an order is set, but its key tmp" + std::to_string(node) + " is not among the outputs of this run");
        keys.push_back(at);
    }
    return m;
}
int order_sort_key(vdl_ctx *c, hipStream_t s, const int64_t *key, uint64_t flip, int64_t m, uint64_t *stw, BufP &perm) {
    HIP_CHECK(hipMemsetAsync(stw, 0, 2 * sizeof(uint64_t), s));
    HIP_CHECK(launch_order_minmax(key, flip, nullptr, m, stw, s));
    int64_t mm[2];
    c->fetch_to_host(stw, 2, mm, s);
    const uint64_t umin = ~(uint64_t)mm[0], range = (uint64_t)mm[1] - umin;
    if (range == 0) return 0;
    const bool split = range >= ((uint64_t)1 << 62);
    int sorts = 0;
    for (int half = split ? 1 : 0; half <= (split ? 2 : 0); half++) {
        const uint64_t top = half == 0 ? range : half == 1 ? 0xffffffffull : range >> 32;
        BufP t = dev_alloc(c, sizeof(int64_t) * (size_t)m);
        HIP_CHECK(launch_order_sortkey(key, flip, perm ? (const int64_t *)perm->p : nullptr, m, umin, half, (int64_t *)t->p, s));
        // (at least two radix passes, so that the slots come out in rank order the way every GROUP BY's Partition leaves them)
        const int64_t pcount = (int64_t)std::max<uint64_t>(top + 1, 512), max_bucket = top + 1 >= 512 ? (int64_t)top : -1;
        BufP scr = dev_alloc(c, partition_scratch_bytes(m, pcount));
        BufP nvalid = dev_alloc(c, sizeof(int64_t));
        BufP ka = dev_alloc(c, sizeof(int64_t) * (size_t)m), sa = dev_alloc(c, sizeof(int64_t) * (size_t)m);
        BufP kb = dev_alloc(c, sizeof(int64_t) * (size_t)m), sb = dev_alloc(c, sizeof(int64_t) * (size_t)m);
        BufP order = dev_alloc(c, sizeof(int64_t) * (size_t)m);
        Src ts; ts.p = t->p; ts.kind = SRC_I64;
        HIP_CHECK(launch_partition(ts, nullptr, m, 0, pcount, scr->p, (uint64_t *)ka->p, (int64_t *)sa->p, (uint64_t *)kb->p, (int64_t *)sb->p,
                                   (int64_t *)nvalid->p, nullptr, s, max_bucket, (int64_t *)order->p, nullptr));
        if (perm) {
            BufP both = dev_alloc(c, sizeof(int64_t) * (size_t)m);
            HIP_CHECK(launch_order_compose((const int64_t *)perm->p, (const int64_t *)order->p, m, (int64_t *)both->p, s));
            perm = both;
        } else perm = order;
        sorts++;
    }
    return sorts;
}
// ---- wide sums: values outside int64 ---------------------------------------------------------------------------------------------
std::string wide_decimal(int64_t lo, int64_t hi) {
    unsigned __int128 u = ((unsigned __int128)(uint64_t)hi << 64) | (uint64_t)lo;
    const bool neg = hi < 0;
    if (neg) u = (unsigned __int128)0 - u;
    std::string s;
    do { s.insert(s.begin(), (char)('0' + (int)(u % 10))); u /= 10; } while (u != 0);
    return neg ? "-" + s : s;
}
// the first value of output o whose high word is not the sign extension of its low word: -1 = every value fits int64
static int64_t wide_first_overflow(const Output &o) {
    const int64_t *lo = o.ptr(), *hi = o.hi_ptr();             // (an output kept in HBM was checked there: GenExec::copy_out_hi)
    if (!lo || !hi) return -1;
    for (size_t i = 0; i < o.count(); i++) if (hi[i] != (lo[i] >> 63)) return (int64_t)i;
    return -1;
}
// checked sums (mode 2): the run fails on the first such value, and delivers nothing
void wide_check_outputs(vdl_plan *p) {
    for (const Output &o : p->outs) {
        const int64_t i = wide_first_overflow(o);
        if (i < 0) continue;
        const std::string msg = "checked sums: output '" + o.name + "' (" + o.tmp + "), group " + std::to_string(i) + ": the exact value " +
                                wide_decimal(o.ptr()[(size_t)i], o.hi_ptr()[(size_t)i]) + " does not fit int64 (vdl_plan_set_wide_sums(plan, 1) delivers it as two words)";
        p->outs.clear();
        throw Error(VDL_ERR_OVERFLOW, msg);
    }
}

void order_outputs_on_host(vdl_ctx *c, vdl_plan *p) {
    std::vector<size_t> keys;
    const int64_t m = order_resolve(p, keys);
    // wide sums: keys are compared as the int64 they are -- a key whose exact value is not one cannot be ordered by it
    for (size_t k : keys) {
        const int64_t i = wide_first_overflow(p->outs[k]);
        if (i < 0) continue;
        const std::string msg = "wide sums: the order key '" + p->outs[k].name + "' (" + p->outs[k].tmp + ") holds, in group " + std::to_string(i) + ", the exact value " +
                                wide_decimal(p->outs[k].ptr()[(size_t)i], p->outs[k].hi_ptr()[(size_t)i]) + ", which does not fit the int64 that keys are compared as";
        p->outs.clear();
        throw Error(VDL_ERR_OVERFLOW, msg);
    }
    const int64_t L = p->order.limit > 0 ? std::min<int64_t>(p->order.limit, m) : m;
    // text keys: an index that has to be built is built (and timed under its own label) before the step's clock starts
    const int n_text = p->order.n_text();
    for (size_t k = 0; n_text > 0 && k < keys.size(); k++)
        if (!p->order.text[k].empty()) collation_ensure(c, p->order.text[k], p, "order key '" + p->outs[keys[k]].name + "'");
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<const int64_t *> kp;
    for (size_t k : keys) kp.push_back(p->outs[k].ptr());
    // ... and the handful of codes goes to the device index and comes back as ranks: one definition of the text order
    std::vector<std::vector<int64_t>> ranks(keys.size());
    if (n_text > 0 && m > 0) {
        hipStream_t s = c->stream;
        std::vector<BufP> codes(keys.size());
        std::vector<const int64_t *> dev(keys.size(), nullptr);
        for (size_t k = 0; k < keys.size(); k++) {
            if (p->order.text[k].empty()) continue;
            codes[k] = dev_alloc(c, sizeof(int64_t) * (size_t)m);
            HIP_CHECK(hipMemcpyAsync(codes[k]->p, kp[k], sizeof(int64_t) * (size_t)m, hipMemcpyHostToDevice, s));
            dev[k] = (const int64_t *)codes[k]->p;
        }
        HIP_CHECK(hipStreamSynchronize(s));                            // (pageable sources)
        const std::vector<BufP> out = order_text_ranks(c, p, dev, m, s);
        for (size_t k = 0; k < keys.size(); k++) {
            if (!out[k]) continue;
            ranks[k].resize((size_t)m);
            HIP_CHECK(hipMemcpyAsync(ranks[k].data(), out[k]->p, sizeof(int64_t) * (size_t)m, hipMemcpyDeviceToHost, s));
            kp[k] = ranks[k].data();
        }
        HIP_CHECK(hipStreamSynchronize(s));
    }
    std::vector<int64_t> index((size_t)L);
    const int rc = vdl_order_host((int)kp.size(), kp.data(), p->order.desc.data(), m, p->order.limit, index.data());
    if (rc != VDL_OK) throw Error(rc, "vdl_order_host failed");
    for (Output &o : p->outs) {
        const int64_t *src = o.ptr();
        std::vector<int64_t> cut((size_t)L);
        for (int64_t i = 0; i < L; i++) cut[(size_t)i] = src[index[(size_t)i]];
        o.vals.swap(cut);
        o.big = nullptr; o.big_n = 0;
        if (o.has_hi) {                                        // wide sums: the high words go with their low words
            std::vector<int64_t> cut_hi((size_t)L);
            const int64_t *src_hi = o.big_hi ? o.big_hi : o.hi.data();
            for (int64_t i = 0; i < L; i++) cut_hi[(size_t)i] = src_hi[(size_t)index[(size_t)i]];
            o.hi.swap(cut_hi);
            o.big_hi = nullptr;
        }
    }
    p->order_note = "host m=" + std::to_string(m) + " rows=" + std::to_string(L);
    if (n_text > 0) p->order_note += " text_keys=" + std::to_string(n_text);
    // (no device work but a text key's translation: the entry is the host's own time for the step)
    p->timings.push_back({"timeInMicrosecondsForOrder", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count()});
}


// The fused front of a plan that does not fuse as a whole (ProjPlan, vdl_fuse.h): one scan over the fact table -- two
// passes: count per tile, then write -- produces the statements of `proj.nodes` as SPARSE vectors on one shared selection;
// the per-operator executor starts from them (`over`).  false: the plan has no such front (or it is switched off).
bool run_projection(vdl_ctx *c, vdl_plan *p, std::map<int, DVec> &over) {
    const ProjPlan &J = p->fused.proj;
    if (!J.ok || (p->use_fusion && p->fused.ok) || !p->use_fusion || getenv("VDL_NO_PROJECTION")) return false;
    auto fbp = std::make_shared<FrontBound>();                 // (kept by the plan until its next run: its descriptors are copied asynchronously)
    FrontBound &fb = *fbp;
    bind_front(c, p, fb);
    if (fb.scols.ncol > kMaxSelectCols) return false;          // more deciding columns than the select pass takes: statement by statement
    p->front_keep = fbp;
    MScanCols &cols = fb.cols, &scols = fb.scols;
    MScanDesc &d = *fb.d;
    std::unique_ptr<MScanDesc> &sdesc = fb.sdesc;
    const std::vector<char> &wanted = fb.wanted;
    const std::vector<int> &distinct = fb.distinct;
    const int64_t n = fb.n;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (p->profiling) {
        if (!p->stmt_ev[1]) { HIP_CHECK(hipEventCreate(&p->stmt_ev[0])); HIP_CHECK(hipEventCreate(&p->stmt_ev[1])); }
        e0 = p->stmt_ev[0]; e1 = p->stmt_ev[1];
        HIP_CHECK(hipEventRecord(e0, c->stream));
    }
    try {
        run_prelude_items(c, p, wanted);
    } catch (const NeedGeneralPath &e) {
        // an assumption of a set the front looks up does not hold for this catalog (a semi-join's modulus smaller than its
        // table): no front for this run -- the statements run one by one, which is exact for any data
        p->front_keep.reset();
        p->fallback_note = e.what();
        return false;
    }
    patch_front(p, fb);
    SelP sel = std::make_shared<Sel>();
    sel->n = n;
    int64_t m = 0;
    std::vector<BufP> outs(distinct.size());
    if (n > 0 && !J.never) {
        // ONE kernel (vdl_mscan_body.h: project_front_body): deciding columns, survivors' ranks, where they go (look-back over the tiles'
        // counts) and the output vectors.  How long those are is only known afterwards: the kernel writes nothing beyond the capacity it
        // is given and leaves the survivors' number in pinned memory.  From a plan's second run on the capacity is an eighth more than
        // last time; a first run takes the whole table's length when that is cheap and otherwise counts first (capacity 0: no
        // survivor is fetched or written); a run that came up short is repeated with the exact number.
        sel->bitmap = dev_alloc(c, sizeof(uint64_t) * (size_t)std::max<int64_t>((n + 63) >> 6, 1));
        sdesc->out_ptr[0] = (int64_t *)sel->bitmap->p;
        BufP look = dev_alloc(c, (size_t)project_look_bytes(n)), total = dev_alloc(c, sizeof(int64_t));
        int64_t *back = c->flag_words() ? c->flag_words() + 1 : nullptr;       // the last batch posts the survivors' number there (system-scope store)
        auto room_for = [&](int64_t cap) {
            sel->idx = dev_alloc(c, sizeof(int64_t) * (size_t)std::max<int64_t>(cap, 1));
            d.out_idx = (int64_t *)sel->idx->p;
            for (size_t o = 0; o < distinct.size(); o++) {
                outs[o] = dev_alloc(c, sizeof(int64_t) * (size_t)std::max<int64_t>(cap, 1));
                d.out_ptr[o] = (int64_t *)outs[o]->p;
            }
            d.out_cap = cap;
        };
        auto pass = [&]() -> int64_t {
            if (back) *(volatile int64_t *)back = -1;
            HIP_CHECK(launch_project_front(scols, desc_on_device(c, p, "select", *sdesc), cols, desc_on_device(c, p, "take", d), look->p, (int64_t *)total->p, back,
                                           c->num_cus, c->stream, front_kernel(c, p, "front", [&] { return one_pass_front(scols, *sdesc, cols, d, p->jit_rt_bounds); })));
            // the host goes on as soon as it knows the number -- while the kernel's other batches still fetch their survivors --: what it
            // queues next runs behind the kernel anyway
            int64_t got = 0;
            if (back) { c->wait_flag(back, -1, c->stream); got = *(volatile int64_t *)back; }
            else c->fetch_to_host(total->p, 1, &got, c->stream);
            return got;
        };
        const int64_t per_row = (int64_t)sizeof(int64_t) * (int64_t)(distinct.size() + 1);
        int64_t cap = p->front_m_seen >= 0 ? std::min<int64_t>(n, p->front_m_seen + p->front_m_seen / 8 + 4096)
                                           : (n * per_row <= ((int64_t)1 << 28) ? n : 0);
        room_for(cap);
        m = pass();
        if (m > cap) { room_for(m); m = pass(); }
        p->front_m_seen = m;
    } else {
        sel->idx = dev_alloc(c, sizeof(int64_t));
        for (size_t o = 0; o < distinct.size(); o++) outs[o] = dev_alloc(c, sizeof(int64_t));
    }
    sel->m = m;
    sel->first_slot = -1;
    for (size_t k = 0; k < J.nodes.size(); k++) {
        DVec v;
        v.kind = DVec::SPARSE; v.n = n; v.sel = sel;
        if (J.node_col[k] == -1) { v.data = sel->idx; v.ids = true; }
        else v.data = outs[(size_t)(std::find(distinct.begin(), distinct.end(), J.node_col[k]) - distinct.begin())];
        over[J.nodes[k]] = v;
    }
    p->front_usec = 0;
    if (e0) {
        HIP_CHECK(hipEventRecord(e1, c->stream));
        HIP_CHECK(hipEventSynchronize(e1));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        p->front_usec = (double)ms * 1e3;
    }
    p->front_note = "timeInMicrosecondsForFusedFront_" + J.table + "_" + std::to_string(J.nodes.size()) + "_statement_vectors_" + std::to_string(m) + "_of_" +
                    std::to_string(n) + "_rows_kept_(dimension_side_included)";
    return true;
}

std::string describe_plan(const vdl_plan *p) {
    std::ostringstream o;
    if (p->use_fusion && p->fused.ok) {
        o << "fused: " << p->fused.scans.size() << " scan(s)\n" << describe_fused(p->fused);
        if (p->use_jit) o << "scan kernels specialised for this plan at first run (hiprtc)" << (p->jit_note.empty() ? "" : ": " + p->jit_note) << "\n";
    } else {
        if (!p->fused.ok) o << describe_fused(p->fused);
        if (p->use_jit && p->fused.proj.ok) o << "projection / dimension scans specialised for this plan at first run (hiprtc)" << (p->jit_note.empty() ? "" : ": " + p->jit_note) << "\n";
        else o << "fusion disabled\n";
        o << "general: " << p->prog.order.size() << " statement(s), one kernel per operator\n";
        for (int id : p->prog.order) {
            const Node &n = p->prog.at(id);
            o << "  op " << n.id << " " << op_name(n.op, n.bin) << "\n";
        }
    }
    return o.str();
}

}  // namespace eng
}  // namespace vdl


// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

const char *vdl_version(void) { return "vdl-mi355x 0.1 (gfx950)"; }

int vdl_open(vdl_ctx **out, int device) {
    if (!out) return VDL_ERR_ARG;
    *out = nullptr;
    vdl_ctx *c = new vdl_ctx();
    int rc = guard(c, [&] {
        c->device = device;
        { const char *g = getenv("VDL_BATCH_GROUPED"); c->batch_grouped = g && *g && *g != '0'; }
        { const char *g = getenv("VDL_BATCH_JOINS"); c->batch_joins = g && *g && *g != '0'; }
        { const char *g = getenv("VDL_LOOKUP_IMAGES"); c->lookup_images = g && *g && *g != '0'; }
        if (device >= 0) {
            int count = 0;
            if (hipGetDeviceCount(&count) != hipSuccess || device >= count)
                throw Error(VDL_ERR_DEVICE, "HIP device " + std::to_string(device) + " not available (" + std::to_string(count) + " device(s) visible)");
            HIP_CHECK(hipSetDevice(device));
            hipDeviceProp_t prop;
            HIP_CHECK(hipGetDeviceProperties(&prop, device));
            c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
            c->arch = prop.gcnArchName;
            if (c->arch.find(':') != std::string::npos) c->arch.resize(c->arch.find(':'));      // "gfx950:sramecc+:xnack-" -> "gfx950"
            if (c->arch.empty()) c->arch = "gfx950";
            HIP_CHECK(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
            c->stream = c->own_stream;
        }
    });
    if (rc != VDL_OK) {
        // keep the context so the caller can read the message
        c->device = -1;
    }
    *out = c;
    return rc;
}

void vdl_ctx::wait_flag(int64_t *word, int64_t until_not, hipStream_t s) {
    volatile int64_t *w = word;
    for (unsigned spins = 0; *w == until_not; spins++) {
        __builtin_ia32_pause();
        if ((spins & 0x3fff) == 0x3fff) {                       // every ~16 K polls: is the stream still going?
            const hipError_t e = hipStreamQuery(s);
            if (e == hipSuccess) {                              // idle: the word was written (or never will be: a launch failed)
                if (*w == until_not) throw Error(VDL_ERR_DEVICE, "a kernel that should have reported to the host did not (the stream is idle)");
                break;
            }
            if (e != hipErrorNotReady) throw Error(VDL_ERR_DEVICE, std::string("hipStreamQuery failed: ") + hipGetErrorString(e));
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
}
void vdl_ctx::wait_here(hipStream_t s) {
    int64_t *flag = flag_words();
    if (!flag) { HIP_CHECK(hipStreamSynchronize(s)); return; }
    const int64_t seq = ++post_seq;
    HIP_CHECK(launch_post_words(nullptr, 0, nullptr, flag, seq, s));
    wait_seq(flag, seq, s);
}
void vdl_ctx::fetch_to_host(const void *dev, size_t k, int64_t *out, hipStream_t s) {
    if (k == 0) return;
    int64_t *pin = pinned((int64_t)k), *flag = flag_words();
    if (!pin || !flag) {
        HIP_CHECK(hipMemcpyAsync(out, dev, sizeof(int64_t) * k, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        return;
    }
    const int64_t seq = ++post_seq;
    HIP_CHECK(launch_post_words((const int64_t *)dev, (int64_t)k, pin, flag, seq, s));
    wait_seq(flag, seq, s);
    std::memcpy(out, pin, sizeof(int64_t) * k);
}

void vdl_close(vdl_ctx *c) {
    if (!c) return;
    if (c->device >= 0) {
        (void)hipSetDevice(c->device);
        (void)hipDeviceSynchronize();
        c->comm.reset();
        c->cols.clear();
        c->sorted_state.reset();
        c->pool->trim();
        c->pool->closed = true;
        if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
        if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
        if (c->copy_ev) (void)hipEventDestroy(c->copy_ev);
    }
    delete c;
}

const char *vdl_last_error(const vdl_ctx *c) { return c ? c->err.c_str() : "null context"; }

int vdl_set_stream(vdl_ctx *c, void *hip_stream) {
    if (!c) return VDL_ERR_ARG;
    return guard(c, [&] {
        need_device(c);
        // pool buffers and plan-owned scratch are protected by stream order alone: drain the stream being left (and the
        // copy stream) so that nothing queued there can still touch memory a launch on the new stream is handed
        if (c->stream != (hipStream_t)hip_stream) {
            HIP_CHECK(hipStreamSynchronize(c->stream));
            if (c->copy_stream) HIP_CHECK(hipStreamSynchronize(c->copy_stream));
        }
        c->stream = (hipStream_t)hip_stream;      // 0 is a real choice: the legacy default stream
    });
}

int vdl_use_own_stream(vdl_ctx *c) {
    if (!c) return VDL_ERR_ARG;
    return guard(c, [&] {
        need_device(c);
        if (c->stream != c->own_stream) {
            HIP_CHECK(hipStreamSynchronize(c->stream));
            if (c->copy_stream) HIP_CHECK(hipStreamSynchronize(c->copy_stream));
        }
        c->stream = c->own_stream;
    });
}

// The column's frame-of-reference image (vdl_column_image.h): min, max and shared decimal trailing zeros in one pass, the choice
// on the host, the image in a second pass.  Replaces whatever image the column had; none when it would not be narrower.
static void build_image(vdl_ctx *c, Column &col) {
    col.image = img::Image{};
    col.image_buf.reset();
    col.packed = img::Packed{};
    col.packed_buf.reset();
    if (col.n <= 0 || col.width <= 1) return;
    BufP st = dev_alloc(c, 3 * sizeof(int64_t));
    HIP_CHECK(launch_image_stats(col.dev, col.width, col.n, (unsigned long long *)st->p, c->stream));
    int64_t w3[3] = {};
    c->fetch_to_host(st->p, 3, w3, c->stream);
    const int64_t mn = (int64_t)((uint64_t)w3[0] ^ 0x8000000000000000ull), mx = (int64_t)((uint64_t)w3[1] ^ 0x8000000000000000ull);
    const img::Image im = img::choose(col.width, mn, mx, (int)w3[2]);
    if (!im.width) return;
    BufP buf = dev_alloc(c, (size_t)col.n * (size_t)im.width);
    HIP_CHECK(launch_image_encode(col.dev, col.width, col.n, im.base, im.scale, buf->p, im.width, c->stream));
    // the bit-packed image of the byte image: e' = e - emin in the bit length of emax - emin
    const int64_t emin = (int64_t)(((uint64_t)mn - (uint64_t)im.base) / (uint64_t)im.scale), emax = (int64_t)(((uint64_t)mx - (uint64_t)im.base) / (uint64_t)im.scale);
    const img::Packed pk = img::pack(im, emin, emax);
    BufP pbuf;
    if (pk.bits) {
        pbuf = dev_alloc(c, (size_t)img::packed_dwords(col.n, pk.bits) * 4);
        HIP_CHECK(launch_image_pack(buf->p, im.width, col.n, emin, pk.bits, pbuf->p, c->stream));
    }
    HIP_CHECK(hipStreamSynchronize(c->stream));
    col.image = im;
    col.image_buf = buf;
    col.packed = pk;
    col.packed_buf = pbuf;
}

// The column's step image (vdl_column_image.h Steps), in one pass; none when the column does not qualify -- some step is not 0 or 1,
// or it has no rows or 2^32 and more.  Replaces whatever step image the column had.
static void build_steps(vdl_ctx *c, Column &col) {
    col.steps = img::Steps{};
    col.steps_buf.reset();
    if (!img::steps_rows_ok(col.n)) return;
    const int64_t padded = project_step_groups(col.n);
    BufP buf = dev_alloc(c, (size_t)padded * 12), out = dev_alloc(c, 2 * sizeof(int64_t));
    HIP_CHECK(hipMemsetAsync(out->p, 0, 2 * sizeof(int64_t), c->stream));
    HIP_CHECK(launch_image_steps(col.dev, col.width, col.n, padded, buf->p, (unsigned long long *)out->p, c->stream));
    int64_t w2[2] = {};
    c->fetch_to_host(out->p, 2, w2, c->stream);
    if (w2[0] != 0) return;
    col.steps.present = true;
    col.steps.base = w2[1];
    col.steps_buf = buf;
}
static bool step_images_by_default() {
    const char *e = getenv("VDL_STEP_IMAGES");
    return e && *e && *e != '0';
}

static void check_width(int w) {
    if (w != 1 && w != 2 && w != 4 && w != 8) throw Error(VDL_ERR_ARG, "elem_bytes must be 1, 2, 4 or 8");
}

int vdl_register_column(vdl_ctx *c, const char *name, const void *dev_ptr, int elem_bytes, int64_t nrows) {
    if (!c || !name) return VDL_ERR_ARG;
    return guard(c, [&] {
        check_width(elem_bytes);
        if (nrows < 0 || (!dev_ptr && nrows > 0)) throw Error(VDL_ERR_ARG, "bad column pointer / length");
        if (((uintptr_t)dev_ptr) % (uintptr_t)elem_bytes) throw Error(VDL_ERR_ARG, "column pointer is not aligned to its element size");
        Column col; col.dev = dev_ptr; col.width = elem_bytes; col.n = nrows;
        c->cols[name] = col;
        c->catalog_version++;
    });
}

int vdl_upload_column(vdl_ctx *c, const char *name, const void *host_ptr, int elem_bytes, int64_t nrows) {
    if (!c || !name) return VDL_ERR_ARG;
    return guard(c, [&] {
        need_device(c);
        check_width(elem_bytes);
        if (nrows < 0 || (!host_ptr && nrows > 0)) throw Error(VDL_ERR_ARG, "bad column pointer / length");
        Column col; col.width = elem_bytes; col.n = nrows;
        col.owned = dev_alloc(c, (size_t)nrows * (size_t)elem_bytes);
        col.dev = col.owned->p;
        if (nrows) HIP_CHECK(hipMemcpyAsync(col.owned->p, host_ptr, (size_t)nrows * (size_t)elem_bytes, hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
        c->cols[name] = col;
        c->catalog_version++;
    });
}

int vdl_generate_column(vdl_ctx *c, const char *name, int elem_bytes, int64_t row0, int64_t nrows, uint64_t seed,
                        int64_t lo, int64_t hi, int64_t mul, int64_t add) {
    if (!c || !name) return VDL_ERR_ARG;
    return guard(c, [&] {
        need_device(c);
        check_width(elem_bytes);
        if (nrows < 0 || hi < lo) throw Error(VDL_ERR_ARG, "bad generator arguments");
        Column col; col.width = elem_bytes; col.n = nrows;
        col.owned = dev_alloc(c, (size_t)nrows * (size_t)elem_bytes);
        col.dev = col.owned->p;
        HIP_CHECK(launch_gen_column(col.owned->p, elem_bytes, row0, nrows, seed, fnv1a(name), lo, hi, mul, add, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
        build_image(c, col);
        c->cols[name] = col;
        c->catalog_version++;
    });
}

int vdl_encode_column(vdl_ctx *c, const char *name) {
    if (!c || !name) return VDL_ERR_ARG;
    return guard(c, [&] {
        need_device(c);
        auto it = c->cols.find(name);
        if (it == c->cols.end()) throw Error(VDL_ERR_COLUMN, std::string("no column '") + name + "'");
        build_image(c, it->second);
        if (step_images_by_default()) build_steps(c, it->second);      // (VDL_STEP_IMAGES=1: how unmodified callers reach the step images)
        c->catalog_version++;
    });
}

int vdl_encode_steps(vdl_ctx *c, const char *name) {
    if (!c || !name) return VDL_ERR_ARG;
    return guard(c, [&] {
        need_device(c);
        auto it = c->cols.find(name);
        if (it == c->cols.end()) throw Error(VDL_ERR_COLUMN, std::string("no column '") + name + "'");
        build_steps(c, it->second);
        c->catalog_version++;
    });
}

int vdl_column_steps_info(const vdl_ctx *c, const char *name, int *present, int64_t *base, int64_t *groups) {
    if (!c || !name) return VDL_ERR_ARG;
    auto it = c->cols.find(name);
    if (it == c->cols.end()) return VDL_ERR_COLUMN;
    const img::Steps &st = it->second.steps;
    if (present) *present = st.present ? 1 : 0;
    if (base) *base = st.present ? st.base : 0;
    if (groups) *groups = st.present ? img::step_groups(it->second.n) : 0;
    return VDL_OK;
}

int vdl_download_steps_image(vdl_ctx *c, const char *name, uint64_t *heads, uint32_t *anchors, int64_t groups) {
    if (!c || !name || !heads || !anchors) return VDL_ERR_ARG;
    return guard(c, [&] {
        need_device(c);
        const Column &col = find_col(c, name);
        if (!col.steps.present || !col.steps_buf) throw Error(VDL_ERR_ARG, std::string("column '") + name + "' has no step image");
        if (groups != img::step_groups(col.n)) throw Error(VDL_ERR_ARG, "the number of groups does not match the step image");
        const char *image = (const char *)col.steps_buf->p;
        HIP_CHECK(hipMemcpyAsync(heads, image, (size_t)groups * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipMemcpyAsync(anchors, image + (size_t)project_step_groups(col.n) * 8, (size_t)groups * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
    });
}

int vdl_declare_steps_image(vdl_ctx *c, const char *name, int64_t base) {
    if (!c || !name) return VDL_ERR_ARG;
    return guard(c, [&] {
        if (c->device >= 0) throw Error(VDL_ERR_ARG, "step images are declared only on a context without a device (a device builds them)");
        auto it = c->cols.find(name);
        if (it == c->cols.end()) throw Error(VDL_ERR_COLUMN, std::string("no column '") + name + "'");
        if (!img::steps_rows_ok(it->second.n)) throw Error(VDL_ERR_ARG, "a step image needs 1 <= rows < 2^32");
        it->second.steps.present = true; it->second.steps.base = base;
        it->second.steps_buf.reset();
        c->catalog_version++;
    });
}

int vdl_set_step_images(vdl_ctx *c, int on) {
    if (!c) return VDL_ERR_ARG;
    return guard(c, [&] {
        if (c->step_images != (on != 0)) c->catalog_version++;      // bound plans re-bind
        c->step_images = on != 0;
    });
}

int vdl_set_lookup_images(vdl_ctx *c, int on) {
    if (!c) return VDL_ERR_ARG;
    return guard(c, [&] {
        if (c->lookup_images != (on != 0)) c->catalog_version++;      // bound plans re-bind
        c->lookup_images = on != 0;
    });
}

int vdl_declare_column_image(vdl_ctx *c, const char *name, int width, int64_t base, int64_t scale) {
    if (!c || !name) return VDL_ERR_ARG;
    return guard(c, [&] {
        if (c->device >= 0) throw Error(VDL_ERR_ARG, "column images are declared only on a context without a device (a device builds them)");
        if ((width != 1 && width != 2 && width != 4) || scale < 1) throw Error(VDL_ERR_ARG, "width must be 1, 2 or 4 and scale be positive");
        auto it = c->cols.find(name);
        if (it == c->cols.end()) throw Error(VDL_ERR_COLUMN, std::string("no column '") + name + "'");
        if (width >= it->second.width) throw Error(VDL_ERR_ARG, "an image is narrower than its column");
        it->second.image.width = width; it->second.image.base = base; it->second.image.scale = scale;
        it->second.image_buf.reset();
        c->catalog_version++;
    });
}

int vdl_column_image_info(const vdl_ctx *c, const char *name, int *width, int64_t *base, int64_t *scale) {
    if (!c || !name) return VDL_ERR_ARG;
    auto it = c->cols.find(name);
    if (it == c->cols.end()) return VDL_ERR_COLUMN;
    const img::Image &im = it->second.image;
    if (width) *width = im.width;
    if (base) *base = im.width ? im.base : 0;
    if (scale) *scale = im.width ? im.scale : 1;
    return VDL_OK;
}

int vdl_column_packed_info(const vdl_ctx *c, const char *name, int *bits, int64_t *base, int64_t *scale) {
    if (!c || !name) return VDL_ERR_ARG;
    auto it = c->cols.find(name);
    if (it == c->cols.end()) return VDL_ERR_COLUMN;
    const img::Packed &pk = it->second.packed;
    if (bits) *bits = pk.bits;
    if (base) *base = pk.bits ? pk.base : 0;
    if (scale) *scale = pk.bits ? pk.scale : 1;
    return VDL_OK;
}

int vdl_download_packed_image(vdl_ctx *c, const char *name, void *host_ptr, size_t bytes) {
    if (!c || !name || !host_ptr) return VDL_ERR_ARG;
    return guard(c, [&] {
        need_device(c);
        const Column &col = find_col(c, name);
        if (!col.packed.bits || !col.packed_buf) throw Error(VDL_ERR_ARG, std::string("column '") + name + "' has no packed image");
        if (bytes != (size_t)img::packed_dwords(col.n, col.packed.bits) * 4) throw Error(VDL_ERR_ARG, "host buffer size does not match the packed image");
        HIP_CHECK(hipMemcpyAsync(host_ptr, col.packed_buf->p, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
    });
}

int vdl_declare_packed_image(vdl_ctx *c, const char *name, int bits, int64_t base, int64_t scale) {
    if (!c || !name) return VDL_ERR_ARG;
    return guard(c, [&] {
        if (c->device >= 0) throw Error(VDL_ERR_ARG, "packed images are declared only on a context without a device (a device builds them)");
        if (bits < 1 || bits > 32 || scale < 1) throw Error(VDL_ERR_ARG, "bits must lie in 1..32 and scale be positive");
        auto it = c->cols.find(name);
        if (it == c->cols.end()) throw Error(VDL_ERR_COLUMN, std::string("no column '") + name + "'");
        it->second.packed.bits = bits; it->second.packed.base = base; it->second.packed.scale = scale;
        it->second.packed_buf.reset();
        c->catalog_version++;
    });
}

int vdl_set_column_images(vdl_ctx *c, int on) {
    if (!c) return VDL_ERR_ARG;
    return guard(c, [&] {
        if (c->images != (on != 0)) c->catalog_version++;      // bound plans re-bind
        c->images = on != 0;
    });
}

int vdl_drop_column(vdl_ctx *c, const char *name) {
    if (!c || !name) return VDL_ERR_ARG;
    return guard(c, [&] {
        if (!c->cols.erase(name)) throw Error(VDL_ERR_COLUMN, std::string("no column '") + name + "'");
        c->catalog_version++;
    });
}

int vdl_column_info(const vdl_ctx *c, const char *name, int *elem_bytes, int64_t *nrows, const void **dev_ptr) {
    if (!c || !name) return VDL_ERR_ARG;
    auto it = c->cols.find(name);
    if (it == c->cols.end()) return VDL_ERR_COLUMN;
    if (elem_bytes) *elem_bytes = it->second.width;
    if (nrows) *nrows = it->second.n;
    if (dev_ptr) *dev_ptr = it->second.dev;
    return VDL_OK;
}

int vdl_download_column(vdl_ctx *c, const char *name, void *host_ptr, size_t bytes) {
    if (!c || !name || !host_ptr) return VDL_ERR_ARG;
    return guard(c, [&] {
        need_device(c);
        const Column &col = find_col(c, name);
        if (bytes != (size_t)col.n * (size_t)col.width) throw Error(VDL_ERR_ARG, "host buffer size does not match the column");
        if (bytes) HIP_CHECK(hipMemcpyAsync(host_ptr, col.dev, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
    });
}

int vdl_parse(vdl_ctx *c, const char *text, size_t len, vdl_plan **out) {
    if (!c || !text || !out) return VDL_ERR_ARG;
    *out = nullptr;
    return guard(c, [&] {
        std::unique_ptr<vdl_plan> p(new vdl_plan());
        p->ctx = c;
        p->device = c->device;
        p->prog = parse_program(text, len);
        rewrite_program(p->prog);
        p->fused = fuse_program(p->prog);
        { const char *j = getenv("VDL_JIT"); p->use_jit = j && *j && *j != '0'; p->jit_tune = p->use_jit && atoi(j) >= 2; }
        { const char *b = getenv("VDL_JIT_BOUNDS"); p->jit_rt_bounds = b && strcmp(b, "runtime") == 0; }
        { const char *w = getenv("VDL_WIDE_SUMS"); p->wide = w && (strcmp(w, "1") == 0 || strcmp(w, "2") == 0) ? atoi(w) : 0; }
        { const char *w = getenv("VDL_WIDE_SHARDED"); p->wide_sharded = w && strcmp(w, "1") == 0; }
        { const char *w = getenv("VDL_WIDE_TAIL"); p->wide_tail = p->wide && w && strcmp(w, "1") == 0; }
        p->description = describe_plan(p.get());
        *out = p.release();
    });
}

void vdl_plan_free(vdl_plan *p) {
    if (!p) return;
    if (p->device >= 0) (void)hipSetDevice(p->device);
    delete p;
    (void)hipGetLastError();
}

const char *vdl_plan_describe(const vdl_plan *p) { return p ? p->description.c_str() : ""; }
int vdl_plan_is_fused(const vdl_plan *p) { return p && p->use_fusion && p->fused.ok; }
int vdl_plan_set_fusion(vdl_plan *p, int enabled) {
    if (!p) return VDL_ERR_ARG;
    p->use_fusion = enabled != 0;
    p->description = describe_plan(p);
    return VDL_OK;
}
int vdl_plan_set_jit(vdl_plan *p, int enabled) {
    if (!p) return VDL_ERR_ARG;
    if (p->use_jit != (enabled != 0)) p->bound = false;       // the scans are bound again, with or without their specialised kernels
    p->use_jit = enabled != 0;
    p->jit_tune = enabled >= 2;
    p->jit_tuned = false;
    p->description = describe_plan(p);
    return VDL_OK;
}
int vdl_plan_set_jit_bounds(vdl_plan *p, int at_run_time) {
    if (!p) return VDL_ERR_ARG;
    if (p->jit_rt_bounds != (at_run_time != 0)) {             // other code: the scans are bound and built again, the front's passes too
        p->bound = false;
        p->jit_tuned = false;
        p->front_jit.clear();
    }
    p->jit_rt_bounds = at_run_time != 0;
    return VDL_OK;
}
void vdl_jit_counters(int64_t *compiled, int64_t *from_disk, int64_t *from_memory) { vdl::jit::counters(compiled, from_disk, from_memory); }
void vdl_prelude_counters(int64_t *items) { if (items) *items = g_prelude_items.load(); }
const char *vdl_plan_jit_note(const vdl_plan *p) { return p ? p->jit_note.c_str() : ""; }
// "role: columns; role: columns" of the roles that have some, out of one of the three texts the plan keeps per role
static int role_columns(const vdl_plan *p, const char **list, std::string vdl_plan::RoleColumns::*text, std::string &out) {
    if (!p || !list) return VDL_ERR_ARG;
    out.clear();
    for (const auto &r : p->roles)
        if (!(r.second.*text).empty()) out += (out.empty() ? "" : "; ") + r.first + ": " + r.second.*text;
    *list = out.c_str();
    return VDL_OK;
}
int vdl_plan_image_columns(const vdl_plan *p, const char **list) { return role_columns(p, list, &vdl_plan::RoleColumns::image, p->image_list); }
int vdl_plan_lookup_columns(const vdl_plan *p, const char **list) { return role_columns(p, list, &vdl_plan::RoleColumns::lookup, p->lookup_list); }
int vdl_plan_step_columns(const vdl_plan *p, const char **list) { return role_columns(p, list, &vdl_plan::RoleColumns::steps, p->step_list); }
// Builds (hiprtc; no GPU needed) the specialised kernel of every multi-aggregate scan of the plan against the columns
// registered now, without loading or running anything: the note lists each kernel with its code size, or why it failed.
int vdl_plan_jit_check(vdl_ctx *c, vdl_plan *p) {
    if (!c || !p) return VDL_ERR_ARG;
    return guard(c, [&] {
        p->jit_note.clear();
        if (p->wide) {                                         // (wide sums: the units a run would refuse to build are refused here too)
            const std::string why = wide_refusal(p);
            if (!why.empty()) throw Error(VDL_ERR_UNSUPPORTED, why);
        }
        if (!p->fused.ok && p->fused.proj.ok) {
            // the fused front of a plan that does not fuse as a whole: both passes of the projection scan, and the dimension
            // scans its prelude holds
            const FusedPlan &F = p->fused;
            for (size_t k = 0; k < F.prelude.size(); k++) {
                const PreludeItem &it = F.prelude[k];
                const bool semi = it.kind == PreludeItem::SEMI_BITMAP;
                if (!(semi || it.kind == PreludeItem::DIM_BITMAP) || !it.scan) continue;
                MScanCols cols;
                auto d = std::make_unique<MScanDesc>();
                bind_prelude_scan(c, p, k, cols, *d);
                build_pass(c, p, (semi ? "semi" : "dim") + std::to_string(k), select_pass(cols, *d, p->jit_rt_bounds), true);
            }
            FrontBound fb;
            bind_front(c, p, fb);
            build_pass(c, p, "front", one_pass_front(fb.scols, *fb.sdesc, fb.cols, *fb.d, p->jit_rt_bounds), true);
            return;
        }
        jit_check_scans(c, p);
    });
}
// ---- ORDER BY / LIMIT (vdl_plan_set_order) -----------------------------------------------------------------------------------
int vdl_order_host(int n_keys, const int64_t *const *keys, const int *descending, int64_t m, int64_t limit, int64_t *index_out) {
    if (n_keys < 0 || n_keys > kOrdMaxKeys || m < 0 || limit < 0 || (n_keys > 0 && (!keys || !descending)) || (m > 0 && !index_out)) return VDL_ERR_ARG;
    for (int k = 0; k < n_keys; k++) if (!keys[k] && m > 0) return VDL_ERR_ARG;
    const int64_t L = limit > 0 ? std::min(limit, m) : m;
    try {
        // u = key ^ flip: signed order as unsigned order, complemented when descending (no negation: INT64_MIN has none)
        uint64_t flip[kOrdMaxKeys];
        for (int k = 0; k < n_keys; k++) flip[k] = descending[k] ? kOrdFlipDesc : kOrdFlipAsc;
        auto before = [&](int64_t a, int64_t b) {
            for (int k = 0; k < n_keys; k++) {
                const uint64_t ua = (uint64_t)keys[k][a] ^ flip[k], ub = (uint64_t)keys[k][b] ^ flip[k];
                if (ua != ub) return ua < ub;
            }
            return a < b;                                 // ties: the position decides, so the order is total
        };
        if (n_keys == 0) { for (int64_t i = 0; i < L; i++) index_out[i] = i; return VDL_OK; }
        std::vector<int64_t> idx((size_t)m);
        for (int64_t i = 0; i < m; i++) idx[(size_t)i] = i;
        if (L < m) std::partial_sort(idx.begin(), idx.begin() + L, idx.end(), before);
        else std::sort(idx.begin(), idx.end(), before);
        std::copy(idx.begin(), idx.begin() + L, index_out);
    } catch (const std::bad_alloc &) { return VDL_ERR_NOMEM; }
    return VDL_OK;
}

int vdl_plan_set_order(vdl_plan *p, int n_keys, const char *const *fields, const int *descending, int64_t limit) {
    if (!p) return VDL_ERR_ARG;
    auto fail = [&](const std::string &why) { if (p->ctx) p->ctx->err = "vdl_plan_set_order: " + why; return (int)VDL_ERR_ARG; };
    if (n_keys < 0) return fail("negative number of keys");
    if (n_keys > kOrdMaxKeys) return fail(std::to_string(n_keys) + " keys given, at most " + std::to_string(kOrdMaxKeys) + " are supported");
    if (limit < 0) return fail("negative limit " + std::to_string(limit));
    if (n_keys > 0 && (!fields || !descending)) return fail("keys without fields / directions");
    vdl_plan::OrderSpec spec;
    for (int k = 0; k < n_keys; k++) {
        const std::string f = fields[k] ? fields[k] : "";
        int node = -1;
        for (int id : p->prog.outputs)
            if (p->prog.at(id).field == f || "tmp" + std::to_string(id) == f) { node = id; break; }
        if (node < 0) return fail("'" + f + "' is not an output of this plan (outputs are named by their full field name or their tmpN key)");
        if (std::find(spec.nodes.begin(), spec.nodes.end(), node) != spec.nodes.end()) return fail("'" + f + "' is given twice");
        spec.nodes.push_back(node);
        spec.desc.push_back(descending[k] != 0);
    }
    spec.text.assign(spec.nodes.size(), std::string());      // a new order carries no text marks (vdl_plan_set_order_text)
    spec.limit = limit;
    spec.set = n_keys > 0 || limit > 0;
    p->order = spec;
    p->order_note.clear();
    return VDL_OK;
}
int vdl_plan_set_order_text(vdl_plan *p, const char *field, const char *heap_column) {
    if (!p) return VDL_ERR_ARG;
    auto fail = [&](const std::string &why) { if (p->ctx) p->ctx->err = "vdl_plan_set_order_text: " + why; return (int)VDL_ERR_ARG; };
    const std::string f = field ? field : "";
    if (heap_column && !*heap_column) return fail("empty heap column name (NULL clears the mark)");
    for (size_t k = 0; k < p->order.nodes.size(); k++) {
        const int id = p->order.nodes[k];
        if (p->prog.at(id).field != f && "tmp" + std::to_string(id) != f) continue;
        p->order.text[k] = heap_column ? heap_column : "";
        return VDL_OK;
    }
    return fail("'" + f + "' is not a key of the order set on this plan" + (p->order.nodes.empty() ? " (no order with keys is set)" : ""));
}
const char *vdl_plan_order_note(const vdl_plan *p) { return p ? p->order_note.c_str() : ""; }
int vdl_plan_set_order_sharded(vdl_plan *p, int on) {
    if (!p) return VDL_ERR_ARG;
    p->order.sharded = on != 0;
    return VDL_OK;
}
int vdl_order_merge_host(int world, int n_keys, const int64_t *counts, const uint64_t *words, int64_t limit, int64_t *run_out, int64_t *index_out, int64_t *n_out) {
    if (world < 1 || world > kMaxExWorld || n_keys < 0 || n_keys > kOrdMaxKeys || !counts || limit < 0) return VDL_ERR_ARG;
    OrdRuns R;
    R.world = world; R.nk = n_keys;
    for (int r = 0; r < world; r++) {
        if (counts[r] < 0) return VDL_ERR_ARG;
        R.off[r + 1] = R.off[r] + counts[r];
    }
    const int64_t N = R.off[world], L = limit > 0 ? std::min(limit, N) : N;
    if ((N > 0 && n_keys > 0 && !words) || (L > 0 && (!run_out || !index_out))) return VDL_ERR_ARG;
    int r = 0;
    for (int64_t j = 0; j < N; j++) {
        while (j >= R.off[r + 1]) r++;
        const int64_t place = ord_merge_place(R, words, j);
        if (place < L) { run_out[place] = r; index_out[place] = j - R.off[r]; }
    }
    if (n_out) *n_out = L;
    return VDL_OK;
}

int vdl_plan_set_device_outputs(vdl_plan *p, int enabled) {
    if (!p) return VDL_ERR_ARG;
    p->device_outputs = enabled != 0;
    return VDL_OK;
}
int vdl_output_device(const vdl_plan *p, int k, const int64_t **dev_vals, size_t *n) {
    if (!p || k < 0 || k >= (int)p->outs.size()) return VDL_ERR_ARG;
    const Output &o = p->outs[(size_t)k];
    if (dev_vals) *dev_vals = o.dev;
    if (n) *n = o.count();
    return VDL_OK;
}
// ---- wide sums ----------------------------------------------------------------------------------------
int vdl_plan_set_wide_sums(vdl_plan *p, int mode) {
    if (!p || mode < 0 || mode > 2) return VDL_ERR_ARG;
    if ((p->wide != 0) != (mode != 0)) {                       // other kernels, other partials: the scans are bound and built again
        p->bound = false;
        p->jit_tuned = false;
        p->wide_note.clear();
    }
    p->wide = mode;
    if (mode == 0) p->wide_sharded = p->wide_tail = false;     // (the sharded and tail switches say how a WIDE plan runs: they go with the mode)
    return VDL_OK;
}
int vdl_plan_set_wide_sums_tail(vdl_plan *p, int on) {
    if (!p) return VDL_ERR_ARG;
    p->wide_tail = p->wide != 0 && on != 0;                   // (it says how a WIDE plan runs: in mode 0 there is nothing to switch)
    return VDL_OK;
}
int vdl_plan_wide_sums_tail(const vdl_plan *p) { return p && p->wide_tail ? 1 : 0; }
int vdl_output_high_device(const vdl_plan *p, int k, const int64_t **dev_hi, size_t *n) {
    if (!p || k < 0 || k >= (int)p->outs.size()) return VDL_ERR_ARG;
    const Output &o = p->outs[(size_t)k];
    if (dev_hi) *dev_hi = o.has_hi && o.dev ? o.dev_hi : nullptr;
    if (n) *n = o.count();
    return VDL_OK;
}
int vdl_wide_join_halves(int64_t sl, int64_t sh, int64_t *lo, int64_t *hi) {
    if (!lo || !hi) return VDL_ERR_ARG;
    wide_join_halves(sl, sh, lo, hi);
    return VDL_OK;
}
int vdl_plan_wide_sums(const vdl_plan *p) { return p ? p->wide : 0; }
int vdl_plan_set_wide_sums_sharded(vdl_plan *p, int on) {
    if (!p) return VDL_ERR_ARG;
    p->wide_sharded = on != 0;
    return VDL_OK;
}
int vdl_plan_wide_sums_sharded(const vdl_plan *p) { return p && p->wide_sharded ? 1 : 0; }
int vdl_output_high(const vdl_plan *p, int k, const int64_t **hi, size_t *n) {
    if (!p || k < 0 || k >= (int)p->outs.size()) return VDL_ERR_ARG;
    const Output &o = p->outs[(size_t)k];
    if (hi) *hi = o.hi_ptr();
    if (n) *n = o.count();
    return VDL_OK;
}
const char *vdl_plan_wide_note(const vdl_plan *p) { return p ? p->wide_note.c_str() : ""; }
int vdl_wide_eval_bin(int op, int64_t alo, int64_t ahi, int64_t blo, int64_t bhi, int64_t *lo, int64_t *hi) {
    if (op < 0 || op >= B_COUNT || !lo || !hi) return VDL_ERR_ARG;
    const wide_t a = (wide_t)(((unsigned __int128)(uint64_t)ahi << 64) | (uint64_t)alo), b = (wide_t)(((unsigned __int128)(uint64_t)bhi << 64) | (uint64_t)blo);
    const unsigned __int128 r = (unsigned __int128)apply_bin_wide(op, a, b);
    *lo = (int64_t)(uint64_t)r;
    *hi = (int64_t)(uint64_t)(r >> 64);
    return VDL_OK;
}
int vdl_plan_set_trace(vdl_plan *p, int enabled) {
    if (!p) return VDL_ERR_ARG;
    p->tracing = enabled != 0;
    if (!p->tracing) p->traced.clear();
    return VDL_OK;
}
int vdl_n_traced(const vdl_plan *p) { return p ? (int)p->traced.size() : 0; }
int vdl_traced(const vdl_plan *p, int k, int *node_id, const char **form, int64_t *n, const int64_t **vals, const uint8_t **ok) {
    if (!p || k < 0 || k >= (int)p->traced.size()) return VDL_ERR_ARG;
    const Traced &t = p->traced[(size_t)k];
    if (node_id) *node_id = t.node;
    if (form) *form = t.form;
    if (n) *n = t.n;
    if (vals) *vals = t.have ? t.vals.data() : nullptr;
    if (ok) *ok = t.have ? t.ok.data() : nullptr;
    return VDL_OK;
}
int vdl_plan_set_profiling(vdl_plan *p, int enabled) {
    if (!p) return VDL_ERR_ARG;
    p->profiling = enabled != 0;
    return VDL_OK;
}

// abandoned: the fused plan is known not to hold for this data (a grouped batch found keys outside the pivots: run_batches) -- the
// general path at once, with that reason, instead of a fused pass that would find the same rows
static int run_plan(vdl_ctx *c, vdl_plan *p, const std::string *abandoned) {
    if (!c || !p) return VDL_ERR_ARG;
    return guard(c, [&] {
        need_device(c);
        p->order_note.clear();
        p->batch_note.clear();
        p->batch_code_bytes = 0;
        if (p->wide) {
            // wide sums are served by the fused aggregate scans alone: refused here, before any kernel runs, where the plan's sums
            // would be computed by anything else
            p->outs.clear();
            const std::string why = wide_refusal(p);
            if (!why.empty()) { p->wide_note = "refused: " + why; throw Error(VDL_ERR_UNSUPPORTED, why); }
            wide_note_merged(p, 0);                            // (an unsharded run: a sharded one's "merged over N ranks" goes)
        }
        if (abandoned) p->fallback_note = *abandoned;
        else if (p->use_fusion && p->fused.ok) {
            const int64_t nw = plan_words(p, nullptr, nullptr);
            if (!p->words || p->words_cap < nw) { p->words = dev_alloc(c, sizeof(int64_t) * (size_t)std::max<int64_t>(nw, 1)); p->words_cap = nw; }
            try {
                run_fused_local(c, p, (int64_t *)p->words->p, true);
                finalize_begin(c, p, (const int64_t *)p->words->p, 0);
                finalize_end(c, p, 0);
                if (p->wide == 2) wide_check_outputs(p);
                if (p->order.set) order_outputs_on_host(c, p);     // a fused plan's outputs are assembled on the host: a handful of rows
                return;
            } catch (const NeedGeneralPath &e) {
                p->fallback_note = e.what();          // exact for any data: rerun statement by statement
            }
            if (p->wide && !p->wide_tail) {
                const std::string why = "wide sums are on, and this run of the fused plan cannot stand: " + p->fallback_note + ".  The statement-by-statement rerun computes its sums with "
                                        "k_group_fold / k_seg_fold / k_fold_global, which have no wide form; clear the switch (vdl_plan_set_wide_sums(plan, 0)) to run it";
                p->wide_note = "refused: " + why;
                p->fallback_note.clear();
                p->outs.clear();
                throw Error(VDL_ERR_UNSUPPORTED, why);
            }
        }
        std::map<int, DVec> over;
        bool front = false;
        if (p->after_front) {
            // a sharded run: whatever happens to the front here, this rank takes part in the collective that follows it
            std::string failure;
            try { front = run_projection(c, p, over); } catch (const Error &e) { failure = e.what(); }
            p->after_front(c, p, over, front, failure);
        } else front = run_projection(c, p, over);
        GenExec g(c, p);
        g.ordering = p->order.set;
        g.wide_on = p->wide != 0 && p->wide_tail && !p->after_front;      // (a wide plan without the tail switch was refused above)
        g.run_nodes(p->prog.outputs, front ? &over : nullptr);
        if (front) p->timings.push_back({p->front_note, p->front_usec});
        if (!p->fallback_note.empty()) { p->timings.push_back({"fusedPlanAbandoned: " + p->fallback_note, 0.0}); p->fallback_note.clear(); }
        if (g.wide_on) {
            p->wide_note = g.wide_note();
            if (p->wide == 2) wide_check_outputs(p);           // (outputs on the host; those kept in HBM were checked there)
        }
    });
}

int vdl_run(vdl_ctx *c, vdl_plan *p) { return run_plan(c, p, nullptr); }

// ---- batched runs: plans that differ in their literals alone share one pass over the columns -----------
namespace {
// The grouping half of a batched run (vdl_specialise.cpp says which plans may share a scan and why not): every group cut into batches
// of at most batch_cap plans (grouped scans: batch_group_cap); alone[i] = why plan i runs alone, "" for a plan of a batch.
struct BatchGrouping {
    std::vector<BatchMember> members;
    std::vector<std::string> alone;
    std::vector<std::vector<BatchMember *>> batches;
};
// (joins_on: vdl_set_batch_joins -- members also agree in their prelude's tables and their conditions' literals)
void batch_group(vdl_ctx *c, vdl_plan *const *plans, int n, bool grouped_on, bool joins_on, BatchGrouping &G) {
    std::vector<BatchMember> &members = G.members;
    members.reserve((size_t)n);
    std::vector<std::string> &alone = G.alone;
    alone.assign((size_t)n, std::string());
    for (int i = 0; i < n; i++) {
        vdl_plan *p = plans[i];
        p->batch_note.clear();
        p->batch_code_bytes = 0;
        alone[(size_t)i] = batch_alone_reason(p, grouped_on, joins_on);
        if (!alone[(size_t)i].empty()) continue;
        BatchMember m;
        m.index = i;
        try { batch_bind(c, p, m); } catch (const Error &e) { alone[(size_t)i] = std::string("its scan does not bind (") + e.what() + ")"; continue; }
        members.push_back(std::move(m));
    }
    // groups in the order of their first plan; a plan with no partner says whether it was the columns or the shape
    std::vector<std::vector<BatchMember *>> groups;
    for (BatchMember &m : members) {
        bool placed = false;
        for (auto &g : groups)
            if (g[0]->cols_key == m.cols_key && g[0]->shape_key == m.shape_key && g[0]->prelude_key == m.prelude_key && g[0]->form_key == m.form_key) { g.push_back(&m); placed = true; break; }
        if (!placed) groups.push_back({&m});
    }
    std::vector<std::vector<BatchMember *>> &batches = G.batches;
    for (auto &g : groups) {
        if (g.size() == 1) {
            // (a join scan: a plan of the same columns and code may still build other lookup tables or hold other literals in its conditions)
            bool same_cols = false, same_shape = false, same_tables = false;
            for (const BatchMember &o : members) {
                if (&o == g[0] || o.cols_key != g[0]->cols_key) continue;
                same_cols = true;
                if (o.shape_key != g[0]->shape_key) continue;
                same_shape = true;
                same_tables |= o.prelude_key == g[0]->prelude_key;
            }
            alone[(size_t)g[0]->index] = same_tables  ? "its conditions' literals differ from every other plan's"
                                         : same_shape ? "no other plan of the call builds the same lookup tables"
                                         : same_cols  ? "its filter shapes differ from every other plan's"
                                         : members.size() > 1 ? "no other plan scans the same columns" : "no other plan of the call can share a scan";
            continue;
        }
        const size_t cap = g[0]->grouped ? (size_t)batch_group_cap(*g[0]->desc, g[0]->replicas_alone) : (size_t)batch_cap_asked(g[0]->desc->nagg);
        if (cap < 2 && g[0]->grouped) { for (BatchMember *m : g) alone[(size_t)m->index] = "its group table leaves no room in LDS for a second plan's classes"; continue; }
        if (cap < 2) { for (BatchMember *m : g) alone[(size_t)m->index] = "a scan of " + std::to_string(m->desc->nagg) + " aggregates leaves no room for a second plan's accumulators"; continue; }
        for (size_t at = 0; at < g.size(); at += cap) {
            const size_t k = std::min(cap, g.size() - at);
            if (k == 1) { alone[(size_t)g[at]->index] = "the one plan left over when its group was cut into batches of " + std::to_string(cap); continue; }
            batches.emplace_back(g.begin() + (std::ptrdiff_t)at, g.begin() + (std::ptrdiff_t)(at + k));
        }
    }
}
struct BatchEvents {
    hipEvent_t a = nullptr, b = nullptr;
    hipEvent_t p0 = nullptr, p1 = nullptr;     // a join batch under profiling: around its one prelude
    ~BatchEvents() { for (hipEvent_t e : {a, b, p0, p1}) if (e) (void)hipEventDestroy(e); }
};
// The scan half: batch b of the grouping as ONE scan, slot q's words left at outs[ms[q]->index] -- the caller's pointers (a sharded
// batch: into its send block) or, with outs null, the plans' own word buffers.  Every plan of the batch is given the word layout a
// finalisation reads, and its note; nothing is finalised here.  Returns the kernel's name.
std::string batch_scan_one(vdl_ctx *c, const std::vector<BatchMember *> &ms, size_t b, bool check_only, int64_t *const *outs_given, BatchEvents &ev) {
    const int K = (int)ms.size();
    bool tune = true, profiling = false;
    int64_t *outs[kMaxBatch] = {};
    if (!check_only && !ms[0]->p->fused.prelude.empty()) {
        // a join batch: the members' preludes build the same tables (batch_group), so the first member's builds them ONCE -- the LIKE
        // tables, the dimension bitmaps, the semi-join set, by the code and the kernels a plan alone runs -- and every member's binding
        // is pointed at them.  (NeedGeneralPath: a semi-join set the fused plan cannot stand for; run_batches reruns every member alone)
        vdl_plan *first = ms[0]->p;
        std::vector<char> wanted(first->fused.prelude.size(), 0);
        for (const ScanColumn &sc : scan_columns(first, 0)) if (sc.prelude >= 0) wanted[(size_t)sc.prelude] = 1;
        const std::vector<char> open = batch_open_items(first);
        bool timed = false;
        for (BatchMember *m : ms) timed = timed || m->p->profiling;
        if (timed && !outs_given) { HIP_CHECK(hipEventCreate(&ev.p0)); HIP_CHECK(hipEventCreate(&ev.p1)); HIP_CHECK(hipEventRecord(ev.p0, c->stream)); }
        run_prelude_items(c, first, wanted, &open);
        if (ev.p1) HIP_CHECK(hipEventRecord(ev.p1, c->stream));
        for (BatchMember *m : ms) {
            if (m->p != first) { m->p->prelude_buf = first->prelude_buf; m->p->prelude_n = first->prelude_n; m->p->prelude_rows = first->prelude_rows; }
            patch_prelude(m->p, scan_columns(m->p, 0), m->cols, *m->desc);
        }
    }
    for (int q = 0; q < K; q++) {
        vdl_plan *p = ms[(size_t)q]->p;
        tune = tune && p->jit_tune;
        profiling = profiling || p->profiling;
        if (check_only) continue;
        const MScanDesc &d = *ms[(size_t)q]->desc;
        const bool grouped = ms[(size_t)q]->grouped;
        const int64_t nw = grouped ? d.pcount * (d.nagg + 1) + 1 : d.nagg + 1;
        if (outs_given) outs[q] = outs_given[ms[(size_t)q]->index];
        else {
            if (!p->words || p->words_cap < nw) { p->words = dev_alloc(c, sizeof(int64_t) * (size_t)nw); p->words_cap = nw; }
            outs[q] = (int64_t *)p->words->p;
        }
        p->order_note.clear();
        if (!p->bound || p->bound_version != c->binding_version()) {
            // finalize_begin / finalize_end read the plan's word layout: one global scan, its words first -- or one grouped scan, whose
            // pivots and aggregate count they take from its descriptor.  The plan stays unbound -- its own kernels are built when it is
            // run alone
            p->bound = false;
            p->reduce_ops.clear();
            p->n_words = plan_words(p, &p->reduce_ops, nullptr);
            p->word_offset.assign(grouped ? 0 : 1, 0);
            p->gword_offset.assign(grouped ? 1 : 0, 0);
            if (grouped) p->mdesc.assign(1, d);
            p->batch_words = true;
        }
    }
    if (profiling && !check_only && !outs_given) { HIP_CHECK(hipEventCreate(&ev.a)); HIP_CHECK(hipEventCreate(&ev.b)); }
    std::string name;
    size_t code_bytes = 0;
    try {
        name = batch_scan(c, ms, tune, check_only, outs, ev.a, ev.b, &code_bytes);
    } catch (const Error &e) {
        throw Error(e.code, "plan " + std::to_string(ms[0]->index) + " (batch " + std::to_string(b) + "): " + e.what());
    }
    for (int q = 0; q < K; q++) {
        ms[(size_t)q]->p->batch_note = "batch " + std::to_string(b) + ": slot " + std::to_string(q) + " of " + std::to_string(K) + ", " + name;
        ms[(size_t)q]->p->batch_code_bytes = code_bytes;
    }
    return name;
}
// A batched run: the grouping, each batch as one scan and its plans' finalisation; every other plan runs alone through vdl_run.
// A plan of a grouped batch whose rows carry keys outside the pivots is rerun alone inside the call; its partners keep their answers.
// check_only (vdl_batch_jit_check): the grouping, the builds and the notes, nothing loaded or run.
void run_batches(vdl_ctx *c, vdl_plan *const *plans, int n, bool check_only) {
    BatchGrouping G;
    batch_group(c, plans, n, c->batch_grouped, c->batch_joins, G);
    std::vector<std::string> &alone = G.alone;
    const std::vector<std::vector<BatchMember *>> &batches = G.batches;
    for (size_t b = 0; b < batches.size(); b++) {
        const std::vector<BatchMember *> &ms = batches[b];
        const int K = (int)ms.size();
        BatchEvents ev;
        std::string name;
        try {
            name = batch_scan_one(c, ms, b, check_only, nullptr, ev);
        } catch (const NeedGeneralPath &e) {
            // the shared prelude says that the fused plan does not hold for this data (a semi-join set taken mod N over a longer table): it
            // says so for every member -- each is rerun alone on the general path at once, as a plan whose rows leave the pivots is below
            const std::string why = e.what();
            for (int q = 0; q < K; q++) {
                vdl_plan *p = ms[(size_t)q]->p;
                p->batch_words = false;
                const int rc = run_plan(c, p, &why);
                if (rc != VDL_OK) throw Error(rc, "plan " + std::to_string(ms[(size_t)q]->index) + ": " + c->err);
                p->batch_note = "alone: rerun after batch " + std::to_string(b) + ": " + why;
            }
            continue;
        }
        if (check_only) continue;
        for (int q = 0; q < K; q++) finalize_begin(c, ms[(size_t)q]->p, (const int64_t *)ms[(size_t)q]->p->words->p, 0);
        float ms_scan = 0;
        // (read once, whichever slots finalise: a slot that is rerun alone must not leave its partners a time of 0)
        if (ev.a) { HIP_CHECK(hipEventSynchronize(ev.b)); HIP_CHECK(hipEventElapsedTime(&ms_scan, ev.a, ev.b)); }
        float ms_prelude = 0;
        if (ev.p1) { HIP_CHECK(hipEventSynchronize(ev.p1)); HIP_CHECK(hipEventElapsedTime(&ms_prelude, ev.p0, ev.p1)); }
        std::vector<std::pair<int, std::string>> rerun;             // slots whose rows carry keys outside the pivots, with finalize_end's words
        bool prelude_said = false;
        for (int q = 0; q < K; q++) {
            vdl_plan *p = ms[(size_t)q]->p;
            try {
                finalize_end(c, p, 0);
                p->batch_words = false;
                if (p->order.set) order_outputs_on_host(c, p);
            } catch (const NeedGeneralPath &e) {
                p->batch_words = false;
                rerun.push_back({q, e.what()});
                continue;
            } catch (const Error &e) {
                p->batch_words = false;
                throw Error(e.code, "plan " + std::to_string(ms[(size_t)q]->index) + ": " + e.what());
            }
            // the whole batch kernel's time, under a label of its own: never a per-query figure
            if (ev.a && p->profiling) p->timings.push_back({"timeInMicrosecondsForBatchedScan_" + name, (double)ms_scan * 1e3});
            // (a join batch: its ONE prelude -- the LIKE tables, bitmaps and sets every slot reads --, on the first slot that finalised)
            if (ev.p1 && p->profiling && !prelude_said) { p->timings.push_back({"timeInMicrosecondsForBatchedPrelude", (double)ms_prelude * 1e3}); prelude_said = true; }
        }
        // (after every slot's finalisation: the others keep their answers and notes.  The batch has shown that the plan's fused scan
        // meets keys outside its pivots: the rerun takes the general path at once, as vdl_run does after its own fused pass says so)
        for (const auto &r : rerun) {
            vdl_plan *p = ms[(size_t)r.first]->p;
            const int rc = run_plan(c, p, &r.second);
            if (rc != VDL_OK) throw Error(rc, "plan " + std::to_string(ms[(size_t)r.first]->index) + ": " + c->err);
            p->batch_note = "alone: rerun after batch " + std::to_string(b) + ": " + r.second;
        }
    }
    for (int i = 0; i < n; i++) {
        if (alone[(size_t)i].empty()) continue;
        if (!check_only) {
            const int rc = vdl_run(c, plans[i]);
            if (rc != VDL_OK) throw Error(rc, "plan " + std::to_string(i) + ": " + c->err);
        }
        plans[i]->batch_note = "alone: " + alone[(size_t)i];
    }
}
int batch_args_ok(vdl_ctx *c, vdl_plan *const *plans, int n, const char *who) {
    if (!c) return VDL_ERR_ARG;
    auto fail = [&](const std::string &why) { c->err = std::string(who) + ": " + why; return (int)VDL_ERR_ARG; };
    if (!plans || n < 1) return fail("no plans given");
    for (int i = 0; i < n; i++) {
        if (!plans[i]) return fail("plan " + std::to_string(i) + " is null");
        for (int j = 0; j < i; j++) if (plans[j] == plans[i]) return fail("plans " + std::to_string(j) + " and " + std::to_string(i) + " are the same plan");
    }
    return VDL_OK;
}
}  // namespace

extern "C++" {                 // (engine-internal: declared in vdl_engine_internal.h, called from vdl_comm.cpp)
namespace vdl {
namespace eng {
int batch_args_check(vdl_ctx *c, vdl_plan *const *plans, int n, const char *who) { return batch_args_ok(c, plans, n, who); }
// The local phase of a sharded batch (vdl_comm.cpp: vdl_run_batch_sharded): run_batches' grouping and scan halves over plans whose one
// scan is a global aggregate scan, slot words left at outs[i], no finalisation -- the words are one rank's partial words.  Grouped
// scans are not grouped here whatever vdl_set_batch_grouped says: the grouped batch kernel finishes as a single rank would.  A batch
// whose scan throws fails ITS plans (code and message in `res`) and nobody else's: the caller still owes its peers the collective.
void batch_local_scans(vdl_ctx *c, vdl_plan *const *plans, int n, int64_t *const *outs, std::vector<BatchLocal> &res) {
    res.assign((size_t)n, BatchLocal{});
    BatchGrouping G;
    batch_group(c, plans, n, false, false, G);
    for (size_t b = 0; b < G.batches.size(); b++) {
        const std::vector<BatchMember *> &ms = G.batches[b];
        int rc = VDL_OK;
        std::string why;
        try {
            BatchEvents ev;
            (void)batch_scan_one(c, ms, b, false, outs, ev);
        } catch (const Error &e) { rc = e.code; why = e.what(); }
        catch (const std::bad_alloc &) { rc = VDL_ERR_NOMEM; why = "out of host memory"; }
        catch (const std::exception &e) { rc = VDL_ERR_ARG; why = e.what(); }
        for (const BatchMember *m : ms) {
            BatchLocal &r = res[(size_t)m->index];
            r.batched = true;
            r.rc = rc;
            r.err = why;
            if (rc != VDL_OK) m->p->batch_words = false;
        }
    }
    for (int i = 0; i < n; i++)
        if (!res[(size_t)i].batched) plans[i]->batch_note = "alone: " + G.alone[(size_t)i];
}
}  // namespace eng
}  // namespace vdl
}  // extern "C++"

int vdl_run_batch(vdl_ctx *c, vdl_plan *const *plans, int n) {
    if (const int rc = batch_args_ok(c, plans, n, "vdl_run_batch")) return rc;
    return guard(c, [&] {
        need_device(c);
        run_batches(c, plans, n, false);
    });
}
int vdl_batch_jit_check(vdl_ctx *c, vdl_plan *const *plans, int n) {
    if (const int rc = batch_args_ok(c, plans, n, "vdl_batch_jit_check")) return rc;
    return guard(c, [&] { run_batches(c, plans, n, true); });
}
const char *vdl_plan_batch_note(const vdl_plan *p) { return p ? p->batch_note.c_str() : ""; }
int64_t vdl_plan_batch_code_bytes(const vdl_plan *p) { return p ? (int64_t)p->batch_code_bytes : 0; }
int vdl_set_batch_grouped(vdl_ctx *c, int on) {
    if (!c) return VDL_ERR_ARG;
    c->batch_grouped = on != 0;
    return VDL_OK;
}
int vdl_set_batch_joins(vdl_ctx *c, int on) {
    if (!c) return VDL_ERR_ARG;
    c->batch_joins = on != 0;
    return VDL_OK;
}

int vdl_n_outputs(const vdl_plan *p) { return p ? (int)p->outs.size() : 0; }
int vdl_output(const vdl_plan *p, int k, const char **name, const char **tmp, const int64_t **vals, size_t *n) {
    if (!p || k < 0 || k >= (int)p->outs.size()) return VDL_ERR_ARG;
    const Output &o = p->outs[(size_t)k];
    if (name) *name = o.name.c_str();
    if (tmp) *tmp = o.tmp.c_str();
    if (vals) *vals = o.ptr();
    if (n) *n = o.count();
    return VDL_OK;
}
int vdl_n_timings(const vdl_plan *p) { return p ? (int)p->timings.size() : 0; }
int vdl_timing(const vdl_plan *p, int k, const char **label, double *usec) {
    if (!p || k < 0 || k >= (int)p->timings.size()) return VDL_ERR_ARG;
    if (label) *label = p->timings[(size_t)k].label.c_str();
    if (usec) *usec = p->timings[(size_t)k].usec;
    return VDL_OK;
}
int vdl_plan_scan_stats(const vdl_plan *p, int64_t *rows, int64_t *algo_bytes, double *usec) {
    if (!p) return VDL_ERR_ARG;
    if (rows) *rows = p->scan_rows;
    if (algo_bytes) *algo_bytes = p->scan_bytes;
    if (usec) *usec = p->scan_usec;
    return VDL_OK;
}

int vdl_plan_scan_traffic(vdl_ctx *c, vdl_plan *p, int64_t *bytes_moved, const char **detail) {
    if (!c || !p) return VDL_ERR_ARG;
    return guard(c, [&] {
        need_device(c);
        if (!(p->use_fusion && p->fused.ok)) throw Error(VDL_ERR_UNSUPPORTED, "vdl_plan_scan_traffic serves fused plans");
        p->traffic_detail.clear();
        const int64_t b = scan_bytes_moved(c, p, p->traffic_detail);
        if (bytes_moved) *bytes_moved = b;
        if (detail) *detail = p->traffic_detail.c_str();
    });
}

int vdl_plan_partial_spec(const vdl_plan *p, int64_t *n_words, const int32_t **reduce_ops) {
    if (!p) return VDL_ERR_ARG;
    vdl_plan *q = const_cast<vdl_plan *>(p);
    if (!(p->use_fusion && p->fused.ok)) {
        // not fused: the plan can still be sharded by rows if its outputs hang off global folds (vdl_plan_set_sharded_table)
        std::string why;
        if (!general_partial_spec(p, q->reduce_ops, why)) {
            if (p->ctx) p->ctx->err = "sharded execution needs a fused plan (outputs = global or dense-domain grouped folds) or global folds over the "
                                      "row-sharded table: " + why;
            return VDL_ERR_UNSUPPORTED;
        }
        if (n_words) *n_words = (int64_t)q->reduce_ops.size();
        if (reduce_ops) *reduce_ops = q->reduce_ops.data();
        return VDL_OK;
    }
    q->reduce_ops.clear();
    bool shardable = true;
    const int64_t off = plan_words(p, &q->reduce_ops, &shardable);
    if (!shardable) {
        if (p->ctx) p->ctx->err = "this fused plan builds a semi-join set from every row of a table: it has no sharded route";
        return VDL_ERR_UNSUPPORTED;
    }
    if (n_words) *n_words = off;
    if (reduce_ops) *reduce_ops = q->reduce_ops.data();
    return VDL_OK;
}

int vdl_run_local(vdl_ctx *c, vdl_plan *p, void *dev_partials) {
    if (!c || !p || !dev_partials) return VDL_ERR_ARG;
    return guard(c, [&] {
        refuse_order_sharded(p);
        refuse_wide_sharded(p, "vdl_run_local");
        need_device(c);
        if (!(p->use_fusion && p->fused.ok)) { general_run_local(c, p, (int64_t *)dev_partials); return; }
        bool shardable = true;
        plan_words(p, nullptr, &shardable);
        if (!shardable) throw Error(VDL_ERR_UNSUPPORTED, "this fused plan builds a semi-join set from every row of a table: it has no sharded route");
        run_fused_local(c, p, (int64_t *)dev_partials, false);
    });
}

int vdl_finalize(vdl_ctx *c, vdl_plan *p, const void *dev_partials) {
    if (!c || !p || !dev_partials) return VDL_ERR_ARG;
    return guard(c, [&] {
        refuse_wide_sharded(p, "vdl_finalize");
        need_device(c);
        if (!(p->use_fusion && p->fused.ok)) { general_finalize(c, p, (const int64_t *)dev_partials); return; }
        finalize_begin(c, p, (const int64_t *)dev_partials, 0);
        finalize_end(c, p, 0);
    });
}

int vdl_plan_set_sharded_table(vdl_plan *p, const char *table) {
    if (!p) return VDL_ERR_ARG;
    p->sharded_table = table ? table : "";
    return VDL_OK;
}
int vdl_plan_set_row_offset(vdl_plan *p, int64_t row0) {
    if (!p) return VDL_ERR_ARG;
    p->row_offset = row0;
    p->bound = false;
    return VDL_OK;
}

int vdl_resolve_first(vdl_ctx *c, vdl_plan *p, void *dev_partials) {
    if (!c || !p || !dev_partials) return VDL_ERR_ARG;
    return guard(c, [&] {
        refuse_wide_sharded(p, "vdl_resolve_first");
        need_device(c);
        if (!(p->use_fusion && p->fused.ok) || !p->bound) throw Error(VDL_ERR_ARG, "vdl_resolve_first needs a fused plan after vdl_run_local");
        const size_t ns = p->fused.scans.size();
        for (size_t g = 0; g < p->fused.gscans.size(); g++) {
            bool any = false;
            for (const ScanAgg &ag : p->fused.gscans[g].aggs) any |= ag.kind == AGG_FIRST;
            if (!any) continue;
            HIP_CHECK(launch_mscan_resolve_first(p->mcols[ns + g], p->mdesc[ns + g], desc_on_device(c, p, "scan" + std::to_string(ns + g), p->mdesc[ns + g]),
                                                 (int64_t *)dev_partials + p->gword_offset[g], c->stream));
        }
    });
}

int vdl_finalize_begin(vdl_ctx *c, vdl_plan *p, const void *dev_partials, int slot) {
    if (!c || !p || !dev_partials) return VDL_ERR_ARG;
    return guard(c, [&] {
        refuse_wide_sharded(p, "vdl_finalize_begin");
        need_device(c);
        if (!(p->use_fusion && p->fused.ok)) { general_finalize(c, p, (const int64_t *)dev_partials); return; }   // nothing left for _end
        finalize_begin(c, p, (const int64_t *)dev_partials, slot);
    });
}

int vdl_finalize_end(vdl_ctx *c, vdl_plan *p, int slot) {
    if (!c || !p) return VDL_ERR_ARG;
    return guard(c, [&] {
        refuse_wide_sharded(p, "vdl_finalize_end");
        need_device(c);
        if (!(p->use_fusion && p->fused.ok)) return;
        finalize_end(c, p, slot);
    });
}

}  // extern "C"
