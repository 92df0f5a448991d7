// vdl_specialise.cpp -- run-time specialisation of the fused aggregate scans (vdl_jit.cpp compiles; the forms: vdl_scan_form.h):
// binding a scan in a form, building it, choosing a form at bind time (VDL_JIT_LATE) or by timing at the first run (the tuner),
// counting the bytes the chosen form moves, and vdl_plan_jit_check's builds without a GPU.  All of it is host-side orchestration.
#include "vdl_specialise.h"

namespace vdl {
namespace eng {

void count_build(vdl_plan *p, const std::string &role, jit::Origin from) {
    std::pair<int, int> &b = p->jit_builds[role];
    b.first++;
    b.second += from != jit::COMPILED;
}
std::string builds_text(const vdl_plan *p, const std::string &role) {
    const auto it = p->jit_builds.find(role);
    if (it == p->jit_builds.end()) return "";
    return "from cache: " + std::to_string(it->second.second) + " of " + std::to_string(it->second.first) + " builds of " + role + "; ";
}

// Run-time specialisation of one multi-aggregate scan (vdl_jit.cpp): the shape of the precompiled variant the launch
// configuration chose, with exactly this scan's column count, and the descriptor as constants.  On success the kernel, its
// grid (occupancy of the specialised code) and name replace the variant's; on failure the variant stays and the note says why.
// (f.u, where the form names one, replaces the variant's row pairs per lane)
// (rt: the plan's bounds at run time, vdl_plan_set_jit_bounds)
static jit::Shape jit_shape(const MScanCols &cols, const ScanLaunch &cfg, const ScanForm &f, bool rt) {
    jit::Shape sh;
    sh.rt_bounds = rt;
    mscan_variant_shape(cfg, &sh.nc, &sh.u, &sh.vec, &sh.grouped, &sh.der);
    sh.nc = cols.ncol;
    for (int k = 0; k < cols.ncol; k++) sh.der |= cols.kind[k] != VC_DIRECT;
    const char *u = getenv(sh.grouped ? "VDL_JIT_GROUP_U" : "VDL_JIT_U");
    if (u && atoi(u) >= 1 && atoi(u) <= 8) sh.u = atoi(u);
    if (f.u > 0) sh.u = f.u;
    else if (f.kind == ScanForm::PACKED) sh.u = getenv("VDL_JIT_U") ? atoi(getenv("VDL_JIT_U")) : 2;      // (the packed form: up to 16 row pairs per slice)
    return sh;
}
// (",img": some columns are read from their images -- a kernel that moves other bytes than the same form over the catalog columns;
// ",rtb", after the form's suffix: bounds at run time)
// (",limg": a lookup reads the image of its target column, vdl_set_lookup_images)
static std::string jit_name(const jit::Shape &sh, const MScanCols &cols) {
    return "k_mscan_specialised<" + std::to_string(sh.nc) + "," + std::to_string(sh.u) + "," + (sh.vec ? "vec" : "novec") + "," + (sh.grouped ? "grouped" : "global") +
           (sh.der ? ",derived" : "") + (cols.image ? ",img" : "") + (cols.limage ? ",limg" : "") + ">";
}
// (tests, profiles: VDL_JIT_LATE=1|2 forces the staged form -- with that many filter columns read with the tile, 4: all of them -- where a column allows it;
// 5 | 6: the packed form, at 2 row pairs per slice unless VDL_JIT_U says otherwise)
static ScanForm form_asked_for() { return getenv("VDL_JIT_LATE") ? ScanForm::from_code(std::max(1, atoi(getenv("VDL_JIT_LATE")))) : ScanForm{}; }

// a column's name without its table
static std::string short_name(const std::string &name) { return name.substr(name.find('.') == std::string::npos ? 0 : name.find('.') + 1); }
// "l_discount@1 l_quantity@2 l_extendedprice@last": which table columns a staged scan reads when (MsArgs::stages)
static std::string stages_text(const vdl_plan *p, size_t s, const MsArgs &args) {
    const std::vector<ScanColumn> &sc = scan_columns(p, s);
    std::string o;
    for (int k = 0; k < args.ncol && k < (int)sc.size(); k++) {
        const int st = args.stage(k);
        if (!st) continue;
        o += (o.empty() ? "" : " ") + short_name(sc[(size_t)k].name) + "@" + (st == 15 ? std::string("last") : st == 14 ? std::string("lookups") : std::to_string(st));
    }
    return o;
}
// "l_shipdate:12 l_discount:4": the columns a packed form reads from packed images, with their bits per row
static std::string packed_text(const vdl_plan *p, size_t s, const MScanCols &cols) {
    const std::vector<ScanColumn> &sc = scan_columns(p, s);
    std::string o;
    for (int k = 0; k < cols.ncol && (size_t)k < sc.size(); k++)
        if ((cols.packed >> k) & 1u) o += (o.empty() ? "" : " ") + short_name(sc[(size_t)k].name) + ":" + std::to_string(cols.pbits[k]);
    return o;
}
// fraction of a table column's rows inside [lo, hi], from 16 samples of 4096 rows spread over the column
static double sampled_selectivity(vdl_ctx *c, const void *dev, int width, int64_t n, int64_t lo, int64_t hi) {
    if (const char *a = getenv("VDL_JIT_ASSUME_SELECTIVITY")) return atof(a);      // (tests without a GPU: vdl_plan_jit_check of staged builds)
    if (n <= 0 || !dev || c->device < 0) return 1.0;
    const int64_t chunk = std::min<int64_t>(4096, n), pieces = std::max<int64_t>(1, std::min<int64_t>(16, n / chunk));
    std::vector<char> host((size_t)(chunk * width));
    int64_t in = 0, seen = 0;
    for (int64_t k = 0; k < pieces; k++) {
        const int64_t at = pieces > 1 ? (n - chunk) / (pieces - 1) * k : 0;
        if (hipMemcpy(host.data(), (const char *)dev + at * width, (size_t)(chunk * width), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return 1.0; }
        for (int64_t i = 0; i < chunk; i++) {
            const int64_t x = width == 8 ? ((const int64_t *)host.data())[i] : width == 4 ? ((const int32_t *)host.data())[i]
                            : width == 2 ? ((const int16_t *)host.data())[i] : ((const int8_t *)host.data())[i];
            in += x >= lo && x <= hi;
        }
        seen += chunk;
    }
    return seen ? (double)in / (double)seen : 1.0;
}

// Stages of a specialised scan that reads late (MsArgs::stages): the most selective filter column on table columns comes
// with the tile, the other filter columns in order of (sampled) selectivity for the rows still in, then the sources of
// derived columns and of the group key, and last the columns that are only aggregate inputs.  0 = nothing to defer.
static uint64_t staged_columns(vdl_ctx *c, const MScanCols &cols, const MScanDesc &d, bool grouped, uint32_t *lazy_mask, int eager_filters = 1) {
    uint32_t source = 0, used = 0;
    for (int k = 0; k < cols.ncol; k++) {
        if (cols.kind[k] == VC_DIRECT) continue;
        if (cols.kind[k] == VC_FORM) { for (int f = d.dsrc[k]; f < d.dsrc[k] + d.dtests[k]; f++) source |= 1u << d.form[f].col; continue; }
        if (d.dsrc[k] >= 0) source |= 1u << d.dsrc[k];
        if (d.dsrc2[k] >= 0) source |= 1u << d.dsrc2[k];
    }
    if (grouped) {
        for (int k = 0; k < d.nkey; k++) if (d.key[k].kind == KeyStep::LOAD) source |= 1u << d.key[k].col;
        for (int k = 0; k < d.ncomp; k++) source |= 1u << d.comp[k].col;
    }
    for (int j = 0; j < d.nagg; j++) if (d.agg[j].kind != AGG_FIRST) used |= d.agg[j].used;
    std::vector<std::pair<double, int>> filters;
    for (int k = 0; k < cols.ncol; k++)
        if (cols.kind[k] == VC_DIRECT && cols.filtered[k])
            filters.push_back({sampled_selectivity(c, cols.ptr[k], cols.width[k], cols.n, cols.lo[k], cols.hi[k]), k});
    std::sort(filters.begin(), filters.end());
    uint64_t stages = 0;
    uint32_t lazy = 0;
    auto put = [&](int k, int st) { stages |= (uint64_t)st << (4 * k); if (st) lazy |= 1u << k; };
    const bool selective = !filters.empty() && filters[0].first < 0.6;
    // (eager_filters = 2: the second most selective filter column comes with the tile as well -- when the first leaves 14 % of
    // the rows, 71 % of the second's sectors are touched anyway and 16-byte streaming loads beat masked 8-byte ones)
    if (selective)
        for (size_t i = (size_t)std::max(eager_filters, 1); i < filters.size(); i++) put(filters[i].second, (int)std::min<size_t>(i - (size_t)std::max(eager_filters, 1) + 1, 3));
    for (int k = 0; k < cols.ncol; k++) {
        if (cols.kind[k] != VC_DIRECT || cols.filtered[k]) continue;
        if ((source >> k) & 1u) { if (selective) put(k, 14); }
        else if ((used >> k) & 1u) put(k, 15);
    }
    *lazy_mask = lazy;
    return stages;
}

// What a form of a scan runs over -- its binding: columns and descriptor -- and the kernel arguments of the form
struct BoundForm {
    const MScanCols *cols = nullptr;          // the binding the caller handed in or, the packed forms, `own`
    const MScanDesc *desc = nullptr;
    std::shared_ptr<MScanCols> own_cols;
    std::shared_ptr<MScanDesc> own_desc;
    MsArgs args;
};
// Scan s in form f at u row pairs: the binding the form runs over and its arguments, or false and why the form does not exist for
// this scan.  The tuner (build_specialised), the census and vdl_plan_jit_check refuse the same forms for the same reasons.
// The eager, staged and queue forms run over the binding handed in (cols, d: the plan's, or vdl_plan_jit_check's own).
// The packed form (the filter columns from their bit-packed images, the columns that are only aggregate inputs late from their byte
// images; every_column: every column from its packed image, nothing late; a column without a packed image comes from its byte image
// with the stripe) has its own binding -- the packed columns' bounds and factors are those of the packed images.  Only global
// aggregate scans over table columns have it.
static bool bind_form(vdl_ctx *c, const vdl_plan *p, size_t s, bool grouped, const ScanForm &f, int u, const MScanCols &cols, const MScanDesc &d, BoundForm &out,
                      std::string &why) {
    out = BoundForm{};
    if (f.kind != ScanForm::PACKED) {
        out.cols = &cols;
        out.desc = &d;
        out.args = mscan_args(cols);
        if (f.kind == ScanForm::EAGER) return true;
        MsArgs &args = out.args;
        args.stages = staged_columns(c, cols, d, grouped, &args.lazy, f.kind == ScanForm::QUEUE ? 1 : f.eager_filters);
        if (!args.lazy) { why = "no column to read late"; return false; }
        if (f.kind == ScanForm::QUEUE) {
            // the queue form: the most selective filter column with the tile, EVERY other table column for the queued rows
            int eager = 0;
            for (int k = 0; k < cols.ncol; k++) {
                if (cols.kind[k] != VC_DIRECT) continue;
                if (!((args.lazy >> k) & 1u)) { eager++; if (!cols.filtered[k]) { why = "a column that is no filter would come with the tile"; return false; } }
            }
            if (eager != 1) { why = "the queue form wants exactly one filter column with the tile"; return false; }
            args.queued = 1;
            args.stages = 0;
        }
        return true;
    }
    if (grouped || s >= p->fused.scans.size()) { why = "the packed form serves global aggregate scans only, not grouped scans"; return false; }
    const ScanPlan &sp = p->fused.scans[s];
    for (const ScanColumn &sc : sp.cols)
        if (sc.kind != VC_DIRECT) { why = "the packed form serves scans over table columns only, not scans with derived columns"; return false; }
    if (!c->images) { why = "column images are off"; return false; }
    if (u != 1 && u != 2 && u != 4 && u != 8 && u != 16) { why = "the packed form takes 1, 2, 4, 8 or 16 row pairs per slice (a lane's 32 values of a stripe split evenly)"; return false; }
    out.own_cols = std::make_shared<MScanCols>();
    out.own_desc = std::make_shared<MScanDesc>();
    MScanCols &pc = *out.own_cols;
    MScanDesc &pd = *out.own_desc;
    int64_t bpr = 0;
    bind_scan(c, p, s, pc, pd, &bpr, p->row_offset, f.every_column ? 2 : 1);
    pd.block_partials = d.block_partials;
    pd.wide = d.wide;
    out.cols = &pc;
    out.desc = &pd;
    if (pc.ncol > 10) { why = "the packed form takes at most 10 columns"; return false; }
    // (a column without a packed image is read from its byte image -- or itself -- with the stripe)
    if (!pc.packed) { why = f.every_column ? "no column has a packed image the scan may read" : "no filter column has a packed image the scan may read"; return false; }
    out.args = mscan_args(pc);
    if (!f.every_column) {
        MsArgs &args = out.args;
        uint32_t used = 0;
        for (int j = 0; j < pd.nagg; j++) if (pd.agg[j].kind != AGG_FIRST) used |= pd.agg[j].used;
        for (int k = 0; k < pc.ncol; k++)
            if (!((pc.packed >> k) & 1u) && !pc.filtered[k] && ((used >> k) & 1u)) { args.stages |= (uint64_t)15 << (4 * k); args.lazy |= 1u << k; }
        if (!args.lazy) { why = "no column to read late"; return false; }
    }
    return true;
}

// a scan built and loaded in one form
struct Specialised {
    std::shared_ptr<jit::Kernel> k;
    int grid = 0, per_cu = 0;
    ScanForm form;                        // (u: the row pairs per lane it was built at)
    size_t code_bytes = 0;
    std::string name, stages, packed;
    BoundForm b;                          // the binding it was built over -- which becomes the plan's when the form is chosen -- and its arguments
};
// (cols, d: the byte-image binding of the scan -- the plan's, unless the plan runs a packed form: tune_specialised)
static bool build_specialised(vdl_ctx *c, vdl_plan *p, size_t s, bool grouped, const ScanForm &f, const MScanCols &cols, const MScanDesc &d, Specialised &out, std::string &why,
                              bool census = false) {
    out = Specialised{};
    jit::Shape sh = jit_shape(cols, p->mcfg[s], f, p->jit_rt_bounds);
    sh.census = census;
    std::vector<char> code;
    if (!bind_form(c, p, s, grouped, f, sh.u, cols, d, out.b, why)) return false;
    const MsArgs &args = out.b.args;
    const MScanDesc &desc = *out.b.desc;
    sh.wide = desc.wide != 0;                                  // (wide sums: every form accumulates through the body's one process step)
    jit::Origin from = jit::COMPILED;
    if (!jit::compile(jit::mscan_source(args, desc, sh), c->arch, code, why, &from)) { why = why.substr(0, 400); return false; }
    count_build(p, "scan " + std::to_string(s), from);
    // a specialised scan is 10-25 KB of code; ten times that means the compiler did not fold the descriptor (it then sits in
    // scratch memory and every descriptor-driven loop stays): such a build is slower than the precompiled kernel
    if (code.size() > (size_t)96 << 10) { why = "the descriptor did not fold (" + std::to_string(code.size()) + " B of code)"; return false; }
    out.k = jit::load(code, why, jit::entry_name(jit::MSCAN, args, desc, sh));
    if (!out.k) return false;
    int per_cu = 0;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, out.k->fn, 256, mscan_lds_bytes(desc, grouped)) != hipSuccess || per_cu < 1) {
        (void)hipGetLastError();
        per_cu = 2;
    }
    if (per_cu > 8) per_cu = 8;
    const int64_t tile = (int64_t)256 * 2 * sh.u;
    int64_t grid = (int64_t)c->num_cus * per_cu;
    // (the packed form: one wave per stripe of 2048 rows at a time, four per block)
    const int64_t most = f.kind == ScanForm::PACKED ? (img::stripes(out.b.cols->n) + 3) / 4 : out.b.cols->n / tile;
    if (grid > most) grid = most;
    if (grid < 1) grid = 1;
    out.grid = (int)grid; out.per_cu = per_cu; out.code_bytes = code.size(); out.form = f; out.form.u = sh.u;
    out.name = jit_name(sh, *out.b.cols);
    out.name.insert(out.name.size() - 1, std::string(f.suffix()) + (sh.rt_bounds ? ",rtb" : "") + (sh.wide ? ",wide" : ""));
    out.stages = stages_text(p, s, args);
    out.packed = packed_text(p, s, *out.b.cols);
    return true;
}
// the note's words on a built form: "..., read late: ...", ", packed: l_shipdate:12 ..."
static std::string form_text(const Specialised &sp) {
    return (sp.packed.empty() ? "" : ", packed: " + sp.packed) + (sp.stages.empty() ? "" : ", read late: " + sp.stages);
}
// a chosen form's kernel, grid and binding become the scan's (the partials area stays the plan's)
static void install_form(vdl_plan *p, size_t s, const Specialised &sp) {
    int64_t *parts = p->mdesc[s].block_partials;
    p->mcols[s] = *sp.b.cols;
    p->mdesc[s] = *sp.b.desc;
    p->mdesc[s].block_partials = parts;
    p->mcfg[s].grid = sp.grid;
    p->mjit[s] = sp.k;
    p->mjit_form[s] = sp.form;
}
bool specialise_scan(vdl_ctx *c, vdl_plan *p, size_t s, bool grouped, std::string *kname) {
    Specialised sp;
    std::string why;
    // (where the packed form does not exist the note says why)
    const ScanForm late = form_asked_for();
    std::string why_late;
    if (late.kind != ScanForm::EAGER && !build_specialised(c, p, s, grouped, late, p->mcols[s], p->mdesc[s], sp, why_late) && late.kind == ScanForm::PACKED)
        p->jit_note += "scan " + std::to_string(s) + ": no packed form (" + why_late + "); ";
    if (!sp.k && !build_specialised(c, p, s, grouped, ScanForm{}, p->mcols[s], p->mdesc[s], sp, why)) { p->jit_note += "scan " + std::to_string(s) + ": not specialised (" + why + "); "; return false; }
    install_form(p, s, sp);
    *kname = sp.name;
    p->jit_note += "scan " + std::to_string(s) + ": " + sp.name + ", " + std::to_string(sp.code_bytes) + " B of code, " + std::to_string(sp.per_cu) + " blocks/CU" + form_text(sp) + "; " +
                   builds_text(p, "scan " + std::to_string(s));
    return true;
}

struct TimingEvents {                                          // (destroyed on every way out, also a throwing HIP_CHECK)
    hipEvent_t a = nullptr, b = nullptr;
    ~TimingEvents() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};
// a candidate's time is the MEDIAN of five launches after the module's first, and a later candidate only replaces the one
// in hand when it is more than 2 % quicker: forms within the noise of each other no longer swap places from run to run
template <typename Launch>
static float median_launch_ms(vdl_ctx *c, TimingEvents &ev, Launch &&launch) {
    std::vector<float> times;
    for (int rep = 0; rep < 6; rep++) {
        HIP_CHECK(hipEventRecord(ev.a, c->stream));
        launch();
        HIP_CHECK(hipEventRecord(ev.b, c->stream));
        HIP_CHECK(hipEventSynchronize(ev.b));
        float t = 0;
        HIP_CHECK(hipEventElapsedTime(&t, ev.a, ev.b));
        if (rep > 0) times.push_back(t);                    // the first launch of a module pays for its load
    }
    std::sort(times.begin(), times.end());
    return times[times.size() / 2];
}

// vdl_plan_set_jit(plan, 2): at the first run, with the real columns and lookup tables in place, every specialised scan is
// built in up to eleven forms (a second each) -- 2, 3, 4, 6 row pairs per lane, then the staged forms that read late (one or two
// filter columns with the tile) at the winner's and at smaller shapes -- and the quickest of three timed launches stays; for a
// single-aggregate scan the hand-tuned k_scan is timed as well.  Which one wins depends on the registers the specialised
// code needs, on how its blocks fill the CUs and on the filters' selectivity: Q1 at SF100 measured 4.13 / 4.04 / 4.30 /
// 3.96 ms for 2 / 3 / 4 / 6 pairs (staged: 4.1-4.2), Q6 2.7 / 2.5 / 2.4 / 2.5 ms eager, 1.63 staged, 2.38 on k_scan.
void tune_specialised(vdl_ctx *c, vdl_plan *p, int64_t *dev_words) {
    const size_t ns = p->fused.scans.size(), ng = p->fused.gscans.size();
    TimingEvents ev;
    HIP_CHECK(hipEventCreate(&ev.a));
    HIP_CHECK(hipEventCreate(&ev.b));
    auto median_ms = [&](auto &&launch) { return median_launch_ms(c, ev, launch); };
    for (size_t s = 0; s < ns + ng; s++) {
        if (!p->mjit[s]) continue;
        const bool grouped = s >= ns;
        int64_t *out = dev_words + (grouped ? p->gword_offset[s - ns] : p->word_offset[s]);
        // (wide sums: the candidates leave their high words where the run will)
        int64_t *out_hi = p->wide && p->wide_hi ? (int64_t *)p->wide_hi->p + (grouped ? p->gword_offset[s - ns] : p->word_offset[s]) : nullptr;
        Specialised best;
        float best_ms = 0;
        std::string tried;
        // {row pairs per lane (0: the quickest eager shape's), form as ScanForm::from_code}
        // rows per lane first; then, at the winner, at 2 and at 1, the staged form that reads late (fewer rows per lane suit it:
        // its loads depend on each other, and what hides them is more waves, not more loads per wave)
        // (3 = the queue form: one filter column with the tile, the rows still in queued per wave and finished 64 at a time)
        // (4 = every filter column with the tile, only aggregate inputs late: over narrow images the filter columns cost little)
        std::vector<std::pair<int, int>> cands = {{2, 0}, {3, 0}, {4, 0}, {6, 0}, {0, 1}, {3, 1}, {2, 1}, {1, 1}, {3, 2}, {2, 2}, {4, 2}, {4, 3}, {3, 3}, {6, 3},
                                                  {2, 4}, {3, 4}, {4, 4}};
        // VDL_JIT_PIN="u=3,late=2" (profiles: tools/profile_bench.sh runs the form a plain run chose, and nothing else): one candidate
        int pin_u = 0, pin_late = -1;
        if (const char *pin = getenv("VDL_JIT_PIN")) {
            if (const char *q = strstr(pin, "u=")) pin_u = atoi(q + 2);
            if (const char *q = strstr(pin, "late=")) pin_late = atoi(q + 5);
            if (pin_u > 0) cands = {{pin_u, std::max(pin_late, 0)}};
        }
        // then the packed forms (5: filter columns from their bit-packed images, aggregate inputs late; 6: every column packed), at 2 to
        // 16 row pairs per slice (more rows per slice: more late loads in flight, fewer waves), with the same rule.  Not under a pin; VDL_JIT_PACKED=0 leaves them out, =only tries nothing else.
        std::vector<std::pair<int, int>> packed_forms = {{2, 5}, {4, 5}, {8, 5}, {16, 5}, {2, 6}, {4, 6}, {8, 6}};
        const char *packed_env = getenv("VDL_JIT_PACKED");
        if (pin_u > 0 || (packed_env && strcmp(packed_env, "0") == 0)) packed_forms.clear();
        else if (packed_env && strcmp(packed_env, "only") == 0) cands.clear();
        if (!packed_forms.empty()) {                           // (forms the scan does not have are not compiled)
            BoundForm b;
            std::string why;
            if (!bind_form(c, p, s, grouped, ScanForm::from_code(5), 2, p->mcols[s], p->mdesc[s], b, why) &&
                !bind_form(c, p, s, grouped, ScanForm::from_code(6), 2, p->mcols[s], p->mdesc[s], b, why)) packed_forms.clear();
        }
        cands.insert(cands.end(), packed_forms.begin(), packed_forms.end());
        // the forms without a binding of their own run over the scan's byte-image binding: the plan's, or -- a scan that runs the
        // packed form now (VDL_JIT_LATE=5 | 6) -- one made here
        const MScanCols *cols = &p->mcols[s];
        const MScanDesc *desc = &p->mdesc[s];
        MScanCols plain_cols;
        std::unique_ptr<MScanDesc> plain_desc;
        if (p->mjit_form[s].kind == ScanForm::PACKED) {
            plain_desc = std::make_unique<MScanDesc>();
            int64_t bpr = 0;
            bind_scan(c, p, s, plain_cols, *plain_desc, &bpr, p->row_offset);
            plain_desc->block_partials = p->mdesc[s].block_partials;
            plain_desc->wide = p->mdesc[s].wide;
            cols = &plain_cols;
            desc = plain_desc.get();
        }
        int best_u = 0;
        for (auto &cu : cands) {
            const ScanForm f = ScanForm::from_code(cu.second, cu.first ? cu.first : best_u);
            if (f.u <= 0 || (f.kind != ScanForm::PACKED && (int64_t)256 * 2 * f.u > cols->n)) continue;
            if (f.kind == ScanForm::STAGED && f.eager_filters == 1 && cu.first == best_u) continue;      // ({0, 1} ran it)
            Specialised cand;
            std::string why;
            if (!build_specialised(c, p, s, grouped, f, *cols, *desc, cand, why)) continue;
            ScanLaunch cfg = p->mcfg[s];
            cfg.grid = cand.grid;
            HIP_CHECK(hipMemcpyAsync(p->mdev[s]->p, cand.b.desc, sizeof(MScanDesc), hipMemcpyHostToDevice, c->stream));
            const float ms = median_ms([&] { HIP_CHECK(launch_mscan(*cand.b.cols, *cand.b.desc, (const MScanDesc *)p->mdev[s]->p, cfg, grouped, false, out, false, c->stream, cand.k->fn, out_hi)); });
            tried += " u=" + std::to_string(f.u) + f.suffix() + ":" + std::to_string((int)(ms * 1000)) + "us";
            if (!best.k || ms < best_ms * 0.98f) { best = cand; best_ms = ms; }
            if (f.kind == ScanForm::EAGER && (best_u == 0 || cand.k == best.k)) best_u = f.u;       // the staged forms start from the quickest eager shape
        }
        if (!best.k) continue;
        if (!grouped && use_kscan(p->fused.scans[s]) && p->block_partials[s] && pin_u <= 0 && !p->wide) {      // (k_scan has no wide build)
            // the hand-tuned single-aggregate kernel is a candidate too
            const float ms = median_ms([&] {
                HIP_CHECK(launch_scan(p->sargs[s], p->scfg[s], c->stream));
                HIP_CHECK(launch_scan_finish(p->sargs[s].block_partials, p->scfg[s].grid, p->sargs[s].nagg, nullptr, p->sargs[s], out, c->stream));
            });
            tried += std::string(" k_scan:") + std::to_string((int)(ms * 1000)) + "us";
            if (ms < best_ms * 0.98f) {
                p->kscan[s] = 1;
                p->mjit[s] = nullptr;
                p->jit_note += "scan " + std::to_string(s) + " tuned:" + tried + " -> " + scan_kernel_name(p->scfg[s]) + "; " + builds_text(p, "scan " + std::to_string(s));
                if ((int)s == p->dominant) p->dominant_kernel = std::string(scan_kernel_name(p->scfg[s])) + "_grid" + std::to_string(p->scfg[s].grid);
                continue;
            }
        }
        install_form(p, s, best);
        if (p->wide) p->wide_note += "; scan " + std::to_string(s) + " tuned -> " + best.name;      // (the note named the form the scan was bound in)
        p->jit_note += "scan " + std::to_string(s) + " tuned:" + tried + " -> " + best.name + (best.packed.empty() ? "" : " (packed: " + best.packed + ")") +
                       (best.stages.empty() ? "" : " (read late: " + best.stages + ")") + "; " + builds_text(p, "scan " + std::to_string(s));
        if ((int)s == p->dominant)
            p->dominant_kernel = best.name + "_grid" + std::to_string(best.grid) + (grouped ? "_rep" + std::to_string(p->mdesc[s].replicas) : "");
    }
    p->description = describe_plan(p);
}

// HBM bytes one launch of the dominant scan moves, counted rather than modelled.  The memory side fetches whole 128-byte lines,
// one request per line, whatever part of the line the lanes ask for (tools/ubench/fetch_calib: TCC_EA0_RDREQ = lines touched
// for streaming, every-other-sector and random masked 16-byte loads alike; FETCH_SIZE = 64 B per request).  A scan that reads
// every column with the tile moves its algorithmic bytes.  A staged scan (late materialisation) moves the eager columns in
// full plus, per late column, 128 B for every line in which some row was still in when the column was read: a CENSUS build of
// the very form that ran (same rows per lane, same stages; vdl_jit.cpp VDL_CENSUS) counts those lines in one untimed launch
// over the real columns.  detail: "column=bytes ..." for the note.
int64_t scan_bytes_moved(vdl_ctx *c, vdl_plan *p, std::string &detail) {
    if (!p->bound || p->dominant < 0) throw Error(VDL_ERR_ARG, "vdl_plan_scan_traffic: run the (fused) plan first");
    const size_t s = (size_t)p->dominant, ns = p->fused.scans.size();
    const bool grouped = s >= ns;
    const std::vector<ScanColumn> &sc = scan_columns(p, s);
    const bool staged = !(!grouped && p->kscan[s]) && p->mjit[s] && p->mjit_form[s].kind != ScanForm::EAGER;
    int64_t total = 0;
    if (!grouped && p->kscan[s]) {                             // the hand-tuned single-aggregate kernel: its own argument block
        const ScanArgs &a = p->sargs[s];
        for (int k = 0; k < a.ncol; k++) { total += a.n * a.width[k]; detail += short_name(sc[(size_t)k].name) + "=" + std::to_string(a.n * a.width[k]) + " "; }
        detail += "(every column read with the tile)";
        return total;
    }
    if (!staged) {
        const MScanCols &cols = p->mcols[s];
        for (int k = 0; k < cols.ncol; k++)
            if (cols.kind[k] == VC_DIRECT) { total += cols.n * cols.width[k]; detail += short_name(sc[(size_t)k].name) + "=" + std::to_string(cols.n * cols.width[k]) + " "; }
        detail += "(every column read with the tile)";
        return total;
    }
    // the census build of the form that ran, over the same binding.  The packed form: every packed column in whole stripes (its padding
    // included), the late columns' lines counted
    const bool packed_form = p->mjit_form[s].kind == ScanForm::PACKED;
    Specialised cen;
    std::string why;
    if (!build_specialised(c, p, s, grouped, p->mjit_form[s], p->mcols[s], p->mdesc[s], cen, why, true))
        throw Error(VDL_ERR_UNSUPPORTED, std::string("the census build of the ") + (packed_form ? "packed" : "staged") + " scan failed: " + why);
    BufP counts = dev_alloc(c, sizeof(unsigned long long) * kMaxVCols);
    BufP words = dev_alloc(c, sizeof(int64_t) * (size_t)std::max<int64_t>(p->n_words, 1));
    HIP_CHECK(hipMemsetAsync(counts->p, 0, sizeof(unsigned long long) * kMaxVCols, c->stream));
    const MScanCols &cols = *cen.b.cols;
    MScanDesc d = *cen.b.desc;
    d.census = (unsigned long long *)counts->p;
    BufP ddev = dev_alloc(c, sizeof(MScanDesc));
    HIP_CHECK(hipMemcpyAsync(ddev->p, &d, sizeof d, hipMemcpyHostToDevice, c->stream));
    ScanLaunch cfg = p->mcfg[s];
    cfg.grid = cen.grid;
    int64_t *out = (int64_t *)words->p + (grouped ? p->gword_offset[s - ns] : p->word_offset[s]);
    BufP words_hi = d.wide ? dev_alloc(c, sizeof(int64_t) * (size_t)std::max<int64_t>(p->n_words, 1)) : nullptr;
    int64_t *out_hi = words_hi ? (int64_t *)words_hi->p + (grouped ? p->gword_offset[s - ns] : p->word_offset[s]) : nullptr;
    HIP_CHECK(launch_mscan(cols, d, (const MScanDesc *)ddev->p, cfg, grouped, false, out, false, c->stream, cen.k->fn, out_hi));
    unsigned long long lines[kMaxVCols] = {};
    c->fetch_to_host(counts->p, kMaxVCols, (int64_t *)lines, c->stream);
    for (int k = 0; k < cols.ncol; k++) {
        if (cols.kind[k] != VC_DIRECT) continue;
        const bool packed = (cols.packed >> k) & 1u, late = (cen.b.args.lazy >> k) & 1u;
        const int64_t b = packed ? img::packed_dwords(cols.n, cols.pbits[k]) * 4 : late ? (int64_t)lines[k] * 128 : cols.n * cols.width[k];
        total += b;
        detail += short_name(sc[(size_t)k].name) + "=" + std::to_string(b) + (packed ? "(packed: " + std::to_string(cols.pbits[k]) + " bits) " :
                                                                               late ? "(late: " + std::to_string(lines[k]) + " lines of " + std::to_string((cols.n * cols.width[k] + 127) / 128) + ") " : " ");
    }
    detail += "(census of " + cen.name + (packed_form ? ")" : ", full tiles)");
    return total;
}

// Builds (hiprtc; no GPU needed) the specialised kernel of every multi-aggregate scan of the plan against the columns
// registered now, without loading or running anything: the note lists each kernel with its code size, or why it failed.
void jit_check_scans(vdl_ctx *c, vdl_plan *p) {
    if (!p->fused.ok) throw Error(VDL_ERR_UNSUPPORTED, "the plan has no fused scans: " + p->fused.why_not);
    const FusedPlan &F = p->fused;
    const size_t ns = F.scans.size();
    for (size_t s = 0; s < ns + F.gscans.size(); s++) {
        const bool grouped = s >= ns;
        MScanCols cols;
        auto d = std::make_unique<MScanDesc>();
        int64_t bpr = 0;
        bind_scan(c, p, s, cols, *d, &bpr, 0);
        d->wide = p->wide ? 1 : 0;                                   // (the wide units build without a device like the others)
        note_roles(p, "scan" + std::to_string(s), scan_columns(p, s), cols);
        const ScanLaunch cfg = mscan_launch_config(cols, *d, grouped, c->num_cus);
        if (cfg.variant < 0) throw Error(VDL_ERR_UNSUPPORTED, "no scan kernel variant for this shape");
        // the staged, queue or packed form of the same scan (VDL_JIT_LATE as in specialise_scan), refused where the tuner refuses it
        const ScanForm late = form_asked_for();
        jit::Shape sh = jit_shape(cols, cfg, late, p->jit_rt_bounds);
        if (getenv("VDL_JIT_CENSUS")) sh.census = true;              // (tests: the measurement build of a staged scan compiles too)
        sh.wide = d->wide != 0;
        std::vector<char> code;
        std::string log;
        BoundForm b;
        if (!bind_form(c, p, s, grouped, late, sh.u, cols, *d, b, log)) {
            p->jit_note += "scan " + std::to_string(s) + ": not specialised (" + log + "); ";
            continue;
        }
        if (!jit::compile(jit::mscan_source(b.args, *b.desc, sh), c->arch, code, log))
            throw Error(VDL_ERR_UNSUPPORTED, "scan " + std::to_string(s) + " does not build: " + log.substr(0, 2000));
        std::string name = jit_name(sh, *b.cols);
        if (b.args.packed) name.insert(name.size() - 1, late.suffix());
        if (sh.rt_bounds) name.insert(name.size() - 1, ",rtb");
        if (sh.wide) name.insert(name.size() - 1, ",wide");
        p->jit_note += "scan " + std::to_string(s) + ": " + name + (b.args.packed ? " (packed: " + packed_text(p, s, *b.cols) + ")" : "") +
                       (b.args.queued ? " (queue)" : b.args.lazy ? " (late)" : "") + ", " + std::to_string(code.size()) + " B of code; ";
    }
}

// ---- batched runs ------------------------------------------------------------------------------------------------------------
// Which plans share a scan is decided here, next to bind_form: the conditions are the packed form's (one global aggregate scan over
// table columns) plus "the same columns" and "the same generated code under run-time bounds".  With vdl_set_batch_grouped a plan
// whose one scan is a grouped scan over table columns shares a grouped batch by the same rules; a batch never mixes the two kinds
// (their shape keys differ).  With vdl_set_batch_joins the one scan may have derived columns and a prelude: plans then share a batch when,
// beside the above, their preludes build the same tables (batch_prelude_key) and their conditions hold the same literals (batch_form_key).
std::string batch_alone_reason(const vdl_plan *p, bool grouped_on, bool joins_on) {
    if (p->wide) return "wide sums are not batched";
    if (!p->use_fusion || !p->fused.ok) return "the plan is not fused";
    if (!p->use_jit) return "specialisation is off";
    const FusedPlan &F = p->fused;
    if (!F.gscans.empty() && !grouped_on) return "grouped scans are not batched";
    const size_t nscans = F.scans.size() + F.gscans.size();
    if (nscans != 1) return "the plan has " + std::to_string(nscans) + " scans, a batch shares exactly one";
    if (!F.prelude.empty() && !joins_on) return "scans with lookup tables or semi-join sets are not batched";
    for (const ScanColumn &sc : scan_columns(p, 0))
        if (sc.kind != VC_DIRECT && !joins_on) return "scans with derived columns are not batched";
    if (F.gscans.empty() ? F.scans[0].never : F.gscans[0].never) return "its filters can hold for no row: there is nothing to scan";
    return "";
}
int batch_cap(int nagg) { return std::min(kMaxBatch, kMaxBatchWords / (1 + std::max(nagg, 0))); }
// VDL_BATCH_WIDTH=k (tests, A/B runs): no batch of either kind is wider than k
static int batch_width_asked() {
    const char *w = getenv("VDL_BATCH_WIDTH");
    return w && atoi(w) >= 2 ? atoi(w) : kMaxBatch;
}
int batch_cap_asked(int nagg) { return std::min(batch_cap(nagg), batch_width_asked()); }
// (a join batch has the same caps: a join scan keeps up to 12 columns per row in registers beside the slots' accumulators, and the units
// of Q14, Q19, Q12 and Q4 at every width need no more scratch memory than the scan's own unit -- DESIGN.md section 5.12,
// profiles/r26/join_batch_resources.txt; nothing reads a unit's scratch size when it is built)

// ---- what a join batch's members must have in common beside columns and shape ----
static void column_text(std::ostringstream &o, const ScanColumn &sc) {
    o << "{" << sc.name << "," << sc.lo << "," << sc.hi << "," << sc.kind << "," << sc.idx << "," << sc.idx2 << "," << sc.prelude << "," << (sc.order_diff ? 1 : 0);
    for (const FormStep &f : sc.form) o << "," << f.op << "/" << f.col << "/" << f.lo << "/" << f.hi;
    o << "}";
}
// the statements a witness depends on, in text order and renumbered from 0: two programs whose dimension sides read alike give one text
static void witness_text(std::ostringstream &o, const Program &P, int witness) {
    std::vector<char> in(P.nodes.size(), 0);
    std::vector<int> todo{witness};
    auto known = [&](int id) { return id > 0 && (size_t)id < P.nodes.size() && P.nodes[(size_t)id].id == id; };
    while (!todo.empty()) {
        const int id = todo.back();
        todo.pop_back();
        if (!known(id) || in[(size_t)id]) continue;
        in[(size_t)id] = 1;
        const Node &n = P.at(id);
        for (int x : {n.a, n.b, n.c}) todo.push_back(x);
    }
    std::map<int, int> number;
    for (int id : P.order) if (known(id) && in[(size_t)id]) { const int k = (int)number.size(); number[id] = k; }
    auto num = [&](int id) { const auto it = number.find(id); return it == number.end() ? -1 : it->second; };
    for (int id : P.order) {
        if (!known(id) || !in[(size_t)id]) continue;
        const Node &n = P.at(id);
        o << "(" << num(id) << ":" << (int)n.op << "," << n.bin << "," << num(n.a) << "," << num(n.b) << "," << num(n.c) << "," << n.imm0 << "," << n.imm1 << "," << n.imm2 << ","
          << n.column << "," << n.pattern << "," << n.field << ")";
    }
}
// Prelude items a join batch leaves OPEN (every row selected, nothing scanned): the dimension bitmap a semi-join scan tests for the
// very row whose bit it is about to set, when that bitmap is a conjunction of range filters on columns of the plan's own scanned
// table that the plan's scan applies itself, with the same bounds (TPC-H Q4: the quarter filters orders, and the set of orders with a
// late lineitem is built from the lineitems of that quarter's orders).  The set then holds more rows of that table, and the scan's
// own filters drop exactly those: the answer is the same, and the set no longer depends on the bounds that differ between the members.
std::vector<char> batch_open_items(const vdl_plan *p) {
    const FusedPlan &F = p->fused;
    std::vector<char> open(F.prelude.size(), 0);
    const std::vector<ScanColumn> &sc = scan_columns(p, 0);
    const std::string &table = F.gscans.empty() ? F.scans[0].table : F.gscans[0].table;
    for (const ScanColumn &user : sc) {
        if (user.kind != VC_BITS || user.prelude < 0 || F.prelude[(size_t)user.prelude].kind != PreludeItem::SEMI_BITMAP) continue;
        if (user.idx < 0 || sc[(size_t)user.idx].kind != VC_ROWID) continue;                  // (the bit of the row's own id)
        const PreludeItem &semi = F.prelude[(size_t)user.prelude];
        if (!semi.scan || semi.bits_of.substr(0, semi.bits_of.find('.')) != table) continue;
        for (const ScanColumn &b : semi.cols) {
            if (b.kind != VC_BITS || b.prelude < 0 || b.idx != semi.index_col || b.lo != 1 || b.hi != 1) continue;
            const PreludeItem &dim = F.prelude[(size_t)b.prelude];
            if (dim.kind != PreludeItem::DIM_BITMAP || !dim.scan || dim.never || dim.table != table) continue;
            bool applied = !dim.cols.empty();
            for (const ScanColumn &d : dim.cols) {
                bool found = false;
                for (const ScanColumn &own : sc) found |= own.kind == VC_DIRECT && d.kind == VC_DIRECT && own.name == d.name && own.lo == d.lo && own.hi == d.hi;
                applied = applied && found;
            }
            // (no other user of the bitmap: every reference to it is this one)
            int users = 0;
            for (const ScanColumn &o : sc) users += o.prelude == b.prelude;
            for (const PreludeItem &it : F.prelude) for (const ScanColumn &o : it.cols) users += o.prelude == b.prelude;
            if (applied && users == 1) open[(size_t)b.prelude] = 1;
        }
    }
    return open;
}
// The canonical text of every prelude item the plan's one scan refers to -- transitively: a dimension scan looks up earlier items --,
// each under its index: equal text means the items build equal tables, and a scan column's `prelude` names the same item in both plans
static std::string batch_prelude_key(const vdl_plan *p) {
    const FusedPlan &F = p->fused;
    const std::vector<char> open = batch_open_items(p);
    std::vector<char> wanted(F.prelude.size(), 0);
    for (const ScanColumn &sc : scan_columns(p, 0)) if (sc.prelude >= 0) wanted[(size_t)sc.prelude] = 1;
    for (size_t k = F.prelude.size(); k-- > 0;)
        if (wanted[k] && F.prelude[k].scan)
            for (const ScanColumn &sc : F.prelude[k].cols) if (sc.prelude >= 0) wanted[(size_t)sc.prelude] = 1;
    std::ostringstream o;
    for (size_t k = 0; k < F.prelude.size(); k++) {
        if (!wanted[k]) continue;
        const PreludeItem &it = F.prelude[k];
        o << "[" << k << ":" << (int)it.kind << ":";
        if (open[k]) o << "open:" << it.table;                 // (left open: its bounds are the scan's own)
        else if (it.kind == PreludeItem::LIKE_LUT) o << it.heap << ":" << it.pattern;
        else if (it.scan) {
            o << "scan:" << it.table << ":" << (it.never ? 1 : 0) << ":" << it.index_col << ":" << it.modulus << ":" << it.bits_of << ":";
            for (const ScanColumn &sc : it.cols) column_text(o, sc);
        } else witness_text(o, p->prog, it.witness);
        o << "]";
    }
    return o.str();
}
// the leaf bounds of the scan's conditions (VC_FORM), as bound: inside one batch every condition is one function of the row
static std::string batch_form_key(const MScanCols &cols, const MScanDesc &d) {
    std::ostringstream o;
    for (int k = 0; k < cols.ncol; k++) {
        if (cols.kind[k] != VC_FORM) continue;
        o << k << ":";
        for (int f = d.dsrc[k]; f < d.dsrc[k] + d.dtests[k]; f++) o << d.form[f].col << "/" << d.form[f].lo << "/" << d.form[f].hi << ",";
        o << ";";
    }
    return o.str();
}
// A grouped batch of K plans keeps 2^K - 1 class tables per replica in LDS: R x (((2^K - 1) x words) | 1) + 256 + nagg + 1 trash words within
// kGroupLdsWords, R the largest power of two <= 8 that fits.  More slots mean fewer replicas, and the replicas are what keeps the lanes of a
// wave off each other's words when a few groups hold most rows: a width is taken only while it leaves min(the replicas the scan has
// alone, kBatchGroupMinReplicas).  (the constant: see DESIGN.md section 5.12 for what was measured)
constexpr int kBatchGroupMinReplicas = 2;
int batch_group_replicas(const MScanDesc &d, int k) {
    const int64_t words = d.pcount * (d.nagg + 1), tables = (((int64_t)1 << k) - 1) * words;
    for (int r = 8; r >= 1; r >>= 1)
        if ((int64_t)r * (tables | 1) + 256 + d.nagg + 1 <= kGroupLdsWords) return r;
    return 0;
}
int batch_group_cap(const MScanDesc &d, int replicas_alone) {
    for (int k = std::min(kMaxBatchGrouped, batch_width_asked()); k >= 2; k--) {
        const int r = batch_group_replicas(d, k);
        if (r >= 1 && r >= std::min(replicas_alone, kBatchGroupMinReplicas)) return k;
    }
    return 0;
}

// the shape of a batch's kernel in form f: the scan's own shape, with the bounds at run time whatever the plans' own setting
static jit::Shape batch_shape(const BatchMember &m, const ScanForm &f, int k) {
    jit::Shape sh = jit_shape(m.cols, m.cfg, f, true);
    sh.grouped = m.grouped;
    sh.der = m.derived;                                        // (a join batch: vdl_set_batch_joins)
    sh.batch = k;
    return sh;
}
void batch_bind(vdl_ctx *c, vdl_plan *p, BatchMember &m) {
    m.p = p;
    m.desc = std::make_shared<MScanDesc>();
    int64_t bpr = 0;
    m.grouped = !p->fused.gscans.empty();
    bind_scan(c, p, 0, m.cols, *m.desc, &bpr, p->row_offset);      // (a batched plan has exactly one scan: batch_alone_reason)
    m.cfg = mscan_launch_config(m.cols, *m.desc, m.grouped, c->num_cus);      // (grouped: the key's canonical form and the replicas the scan has alone)
    m.replicas_alone = m.desc->replicas;
    for (int i = 0; i < m.cols.ncol; i++) m.derived = m.derived || m.cols.kind[i] != VC_DIRECT;
    if (m.cfg.variant < 0) throw Error(VDL_ERR_UNSUPPORTED, "no multi-aggregate scan kernel variant for this shape");
    std::ostringstream k;
    k << m.cols.ncol << ":" << m.cols.n << ":" << m.cols.row0 << ":" << m.cols.image;
    for (int i = 0; i < m.cols.ncol; i++) k << ":" << m.cols.ptr[i] << "/" << m.cols.width[i];
    m.cols_key = k.str();
    m.shape_key = jit::entry_name(jit::MSCAN, mscan_args(m.cols), *m.desc, batch_shape(m, ScanForm{}, 0));
    m.prelude_key = batch_prelude_key(p);
    m.form_key = batch_form_key(m.cols, *m.desc);
}

}  // namespace eng
}  // namespace vdl

struct vdl::eng::BatchEntry {
    std::shared_ptr<jit::Kernel> k;
    int grid = 0, per_cu = 0;
    ScanForm form;                             // (u: the row pairs per lane / per slice it was built at)
    std::string name, entry;
    size_t code_bytes = 0;
    bool grouped = false;                      // a grouped batch: dynamic LDS for its class tables, [grid][slots][words + 1] partials
    BufP descs, partials;
    size_t partial_words = 0;
    std::vector<unsigned char> shadow;         // what `descs` holds: uploaded again only when some slot's descriptor changed
};

namespace vdl {
namespace eng {

// every member's binding in form f -- packed bounds live in the packed image's domain -- or false and why: the form does not exist for
// a member, or the members' bindings in it do not give ONE code over ONE set of columns (a bound that falls off a packed image's end
// for one plan only is another shape there)
static bool batch_bind_form(vdl_ctx *c, const std::vector<BatchMember *> &ms, const ScanForm &f, const jit::Shape &sh, std::vector<BoundForm> &bound, std::string &entry,
                            std::string &why) {
    const size_t K = ms.size();
    bound.assign(K, BoundForm{});
    for (size_t q = 0; q < K; q++) {
        if (!bind_form(c, ms[q]->p, 0, ms[q]->grouped, f, sh.u, ms[q]->cols, *ms[q]->desc, bound[q], why)) return false;
        const MsArgs &a = bound[q].args, &a0 = bound[0].args;
        const std::string name = jit::entry_name(jit::MSCAN, a, *bound[q].desc, sh);
        if (q == 0) entry = name;
        bool same = name == entry && a.n == a0.n && a.row0 == a0.row0 && a.packed == a0.packed && a.pbits == a0.pbits && a.widths == a0.widths && a.ncol == a0.ncol;
        for (int k = 0; k < a0.ncol && same; k++) same = a.ptr[k] == a0.ptr[k];
        if (!same) { why = "the plans' bindings differ in this form"; return false; }
    }
    return true;
}
// the batch's kernel over the members' bindings: compiled, and unless check_only loaded, with the grid its registers allow
static bool batch_build(vdl_ctx *c, const ScanForm &f, const jit::Shape &sh, const std::vector<BoundForm> &bound, const std::string &entry, bool check_only, BatchEntry &out,
                        std::string &why) {
    const MsArgs &args = bound[0].args;
    const MScanDesc &desc = *bound[0].desc;
    std::vector<char> code;
    if (!jit::compile(jit::mscan_source(args, desc, sh), c->arch, code, why)) { why = why.substr(0, 2000); return false; }
    if (code.size() > (size_t)96 << 10) { why = "the descriptor did not fold (" + std::to_string(code.size()) + " B of code)"; return false; }
    out = BatchEntry{};
    out.form = f; out.form.u = sh.u;
    out.grouped = sh.grouped;
    out.code_bytes = code.size();
    out.entry = entry;
    out.name = jit_name(sh, *bound[0].cols);
    out.name.insert(out.name.size() - 1, std::string(f.suffix()) + ",batch" + std::to_string(sh.batch) + ",rtb");
    if (check_only) return true;
    out.k = jit::load(code, why, entry);
    if (!out.k) return false;
    int per_cu = 0;
    const size_t lds = sh.grouped ? mscan_batch_lds_bytes(desc, sh.batch) : 0;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, out.k->fn, 256, lds) != hipSuccess || per_cu < 1) { (void)hipGetLastError(); per_cu = 2; }
    if (per_cu > 8) per_cu = 8;
    int64_t grid = (int64_t)c->num_cus * per_cu;
    // (the packed form: one wave per stripe of 2048 rows at a time, four per block)
    const int64_t most = f.kind == ScanForm::PACKED ? (img::stripes(args.n) + 3) / 4 : args.n / ((int64_t)256 * 2 * sh.u);
    if (grid > most) grid = most;
    if (grid < 1) grid = 1;
    out.grid = (int)grid; out.per_cu = per_cu;
    return true;
}

// the slots' descriptors on the device (uploaded when they differ from what is there), the partials area, the launch
static void batch_launch(vdl_ctx *c, BatchEntry &e, const std::vector<BoundForm> &bound, int64_t *const *outs) {
    const int K = (int)bound.size(), W = bound[0].desc->nagg + 1;
    std::vector<unsigned char> want(sizeof(MScanDesc) * (size_t)K);
    for (int q = 0; q < K; q++) {
        MScanDesc d = *bound[(size_t)q].desc;
        d.block_partials = nullptr;                            // (the batch has one partials area: MsBatch)
        // the kernel compares a 1- or 2-byte column in 32 bits (eval_pass_narrow): a bound beyond the column's domain says the same one
        // step outside it
        const MsArgs &a = bound[(size_t)q].args;
        for (int k = 0; k < a.ncol; k++) {
            // (a filtered derived column of a join batch is compared in 64 bits: its bounds stay)
            if (!((a.filtered >> k) & 1u) || ((a.packed >> k) & 1u) || ((a.derived >> k) & 1u) || a.width(k) >= 4) continue;
            const int64_t top = ((int64_t)1 << (8 * a.width(k) - 1));
            d.flo[k] = std::min(d.flo[k], top);
            d.fhi[k] = std::max(d.fhi[k], -top - 1);
        }
        std::memcpy(want.data() + sizeof(MScanDesc) * (size_t)q, &d, sizeof d);
    }
    if (!e.descs) e.descs = dev_alloc(c, want.size());
    if (want != e.shadow) {
        e.shadow.swap(want);                                   // (the source of the copy stays put until the next upload)
        HIP_CHECK(hipMemcpyAsync(e.descs->p, e.shadow.data(), e.shadow.size(), hipMemcpyHostToDevice, c->stream));
    }
    const size_t words = (size_t)e.grid * (size_t)K * (e.grouped ? (size_t)(bound[0].desc->pcount * W + 1) : (size_t)W);
    if (!e.partials || e.partial_words < words) { e.partials = dev_alloc(c, sizeof(int64_t) * words); e.partial_words = words; }
    MsBatch b;
    for (int q = 0; q < K; q++) b.d[q] = (const MScanDesc *)e.descs->p + q;
    b.partials = (int64_t *)e.partials->p;
    HIP_CHECK(launch_mscan_batch(*bound[0].cols, *bound[0].desc, b, K, e.grid, outs, c->stream, e.k->fn, e.grouped));
}

std::string batch_scan(vdl_ctx *c, const std::vector<BatchMember *> &ms, bool tune, bool check_only, int64_t *const *outs, hipEvent_t ev0, hipEvent_t ev1,
                       size_t *code_bytes) {
    const int K = (int)ms.size();
    const bool grouped = ms[0]->grouped, derived = ms[0]->derived;
    if (K < 2 || (grouped ? K > kMaxBatchGrouped || batch_group_replicas(*ms[0]->desc, K) < 1 : K > batch_cap(ms[0]->desc->nagg)))
        throw Error(VDL_ERR_ARG, "a batch of " + std::to_string(K) + " plans does not fit the kernel");
    // (a grouped batch is generated for the replicas its width leaves: part of every slot's descriptor from here on)
    if (grouped) for (BatchMember *m : ms) m->desc->replicas = batch_group_replicas(*m->desc, K);
    // VDL_JIT_PIN="u=2,late=6" leaves the tuner one candidate as it does for a plan's own scan: late=6 the packed form, any other value eager
    int pin_u = 0, pin_late = 0;
    const char *pin = tune ? getenv("VDL_JIT_PIN") : nullptr;
    if (pin) {
        if (const char *q = strstr(pin, "u=")) pin_u = atoi(q + 2);
        if (const char *q = strstr(pin, "late=")) pin_late = atoi(q + 5);
    }
    const char *env_u = getenv(grouped ? "VDL_JIT_GROUP_U" : "VDL_JIT_U");
    const std::string key = ms[0]->shape_key + "|" + ms[0]->cols_key + "|" + std::to_string(K) + (tune ? "|tuned|" : "||") + (pin ? pin : "") + "|" + (env_u ? env_u : "") +
                            (c->images ? "|img" : "|") + (check_only ? "|check" : "");
    std::vector<BoundForm> bound;
    std::string why, entry;
    std::shared_ptr<BatchEntry> e;
    auto hit = c->batches.find(key);
    if (hit != c->batches.end()) {
        // the kernel in hand serves these plans when their bindings in its form give its code again (the eager form: always)
        e = hit->second;
        if (!batch_bind_form(c, ms, e->form, batch_shape(*ms[0], e->form, K), bound, entry, why) || entry != e->entry) { c->batches.erase(hit); e = nullptr; }
    }
    if (!e) {
        // {row pairs per lane or slice (0: the launch configuration's), form as ScanForm::from_code}: untuned the eager form as the scan's own
        // shape has it; tuned the eager form at 2, 3, 4 and the every-column packed form at 2, 4, by the tuner's rule; the staged, queue
        // and packed-late forms are not batched
        std::vector<std::pair<int, int>> cands = {{0, 0}};
        // (a grouped batch and a join batch have the eager tile form alone)
        if (tune && pin_u > 0) cands = {{pin_u, pin_late == 6 && !grouped && !derived ? 6 : 0}};
        else if (tune && !check_only && (grouped || derived)) cands = {{2, 0}, {3, 0}, {4, 0}};
        else if (tune && !check_only) cands = {{2, 0}, {3, 0}, {4, 0}, {2, 6}, {4, 6}};
        TimingEvents ev;
        if (cands.size() > 1) { HIP_CHECK(hipEventCreate(&ev.a)); HIP_CHECK(hipEventCreate(&ev.b)); }
        float best_ms = 0;
        std::vector<BoundForm> best_bound;
        std::string first_why;
        for (const auto &cu : cands) {
            const ScanForm f = ScanForm::from_code(cu.second, cu.first);
            const jit::Shape sh = batch_shape(*ms[0], f, K);
            if (cands.size() > 1 && f.kind != ScanForm::PACKED && (int64_t)256 * 2 * sh.u > ms[0]->cols.n) continue;
            auto cand = std::make_shared<BatchEntry>();
            std::vector<BoundForm> cb;
            std::string cwhy, centry;
            if (!batch_bind_form(c, ms, f, sh, cb, centry, cwhy) || !batch_build(c, f, sh, cb, centry, check_only, *cand, cwhy)) {
                if (first_why.empty()) first_why = cwhy;
                continue;
            }
            float ms_ = 0;
            if (cands.size() > 1) ms_ = median_launch_ms(c, ev, [&] { batch_launch(c, *cand, cb, outs); });
            if (!e || ms_ < best_ms * 0.98f) { e = cand; best_ms = ms_; best_bound = cb; }
        }
        if (!e && !(cands.size() == 1 && cands[0] == std::make_pair(0, 0))) {
            // no candidate exists for these plans (a table shorter than a tile, a pinned packed form without packed images): the eager form
            const ScanForm f{};
            const jit::Shape sh = batch_shape(*ms[0], f, K);
            auto cand = std::make_shared<BatchEntry>();
            if (batch_bind_form(c, ms, f, sh, best_bound, entry, why) && batch_build(c, f, sh, best_bound, entry, check_only, *cand, why)) e = cand;
            else first_why = why;
        }
        if (!e) throw Error(VDL_ERR_UNSUPPORTED, "the batched scan does not build: " + first_why);
        bound = best_bound;
        if (c->batches.size() > 256) c->batches.clear();
        c->batches[key] = e;
    }
    if (!check_only) {
        if (ev0) HIP_CHECK(hipEventRecord(ev0, c->stream));
        batch_launch(c, *e, bound, outs);
        if (ev1) HIP_CHECK(hipEventRecord(ev1, c->stream));
    }
    if (code_bytes) *code_bytes = e->code_bytes;
    return e->name;
}

}  // namespace eng
}  // namespace vdl
