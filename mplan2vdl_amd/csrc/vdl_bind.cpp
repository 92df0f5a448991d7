// vdl_bind.cpp -- binding: a planned scan and the catalog's columns become kernel arguments (MScanCols / MScanDesc, ScanArgs).
//
// ONE binder decides, column by column, from which stored form a column is read -- the catalog column, its step image, its byte
// image or its bit-packed image (vdl_column_image.h) -- and in which domain its bounds, its formula tests and its aggregate factors
// live.  What differs between the scan roles is handed to it as data (BindRules); what only one role has -- aggregate factors and the
// group key, the prelude's tables, the front's two sides -- is a short step of that role after the shared loop.  Works on a context
// without a device over declared images (vdl_plan_jit_check).
#include "vdl_engine_internal.h"

namespace vdl {
namespace eng {

// single-aggregate scans over <= 4 columns take the tuned k_scan; everything else k_mscan
bool use_kscan(const ScanPlan &sp) {
    for (const ScanColumn &c : sp.cols) if (c.kind != VC_DIRECT) return false;       // derived columns (fused join scans): k_mscan
    if (getenv("VDL_NO_KSCAN")) return false;                                         // experiments: everything through k_mscan
    return sp.aggs.size() == 1 && sp.cols.size() <= 4;
}

const std::vector<ScanColumn> &scan_columns(const vdl_plan *p, size_t s) {
    const size_t ns = p->fused.scans.size();
    return s < ns ? p->fused.scans[s].cols : p->fused.gscans[s - ns].cols;
}

// A comparison of two columns is planned as a range of their difference (vdl_fuse.cpp mk_cmp_diff: a > b as a - b in [1, max]), read
// for its sign and its zero.  The wrap-around difference (VC_SUB) has them right while a - b stays inside int64: certain when both
// operands are table columns, or lookups of columns, stored in fewer than 8 bytes (TPC-H compares int32 dates this way: those scans
// are what they were).  Over anything wider the bound scan computes the saturated difference instead (VC_SUBS), whose sign and zero
// are those of the exact one for any operands.  (A Subtract the program wrote itself means its wrap-around value and carries no mark.)
static int bound_kind(vdl_ctx *c, const std::vector<ScanColumn> &sc, const ScanColumn &s) {
    if (s.kind != VC_SUB || !s.order_diff) return s.kind;
    for (int src : {s.idx, s.idx2}) {
        const ScanColumn *o = src >= 0 && (size_t)src < sc.size() ? &sc[(size_t)src] : nullptr;
        if (!(o && (o->kind == VC_DIRECT || o->kind == VC_GATHER) && find_col(c, o->name).width < 8)) return VC_SUBS;
    }
    return VC_SUB;
}

// formula columns (VC_FORM) into the descriptor's pool, in the kernels' layout (MScanDesc::form): the range tests sorted by
// column, then the postfix program with every test replaced by a reference to its result bit
static void bind_forms(const std::vector<ScanColumn> &sc, MScanDesc &d) {
    int used = 0;
    for (size_t k = 0; k < sc.size(); k++) {
        if (sc[k].kind != VC_FORM) continue;
        const std::vector<FormStep> &prog = sc[k].form;
        std::vector<int> tests;
        for (size_t i = 0; i < prog.size(); i++) if (prog[i].op == FormStep::LEAF) tests.push_back((int)i);
        std::stable_sort(tests.begin(), tests.end(), [&](int x, int y) { return prog[(size_t)x].col < prog[(size_t)y].col; });
        if (tests.size() > 64 || used + (int)(tests.size() + prog.size()) > kMaxFormPool)
            throw Error(VDL_ERR_UNSUPPORTED, "the scan's conditions do not fit the descriptor (" + std::to_string(kMaxFormPool) + " steps in all, 64 tests per condition)");
        std::vector<int> bit_of(prog.size(), -1);
        d.dsrc[k] = used;
        d.dtests[k] = (int)tests.size();
        for (size_t t = 0; t < tests.size(); t++) { bit_of[(size_t)tests[t]] = (int)t; d.form[used++] = prog[(size_t)tests[t]]; }
        for (size_t i = 0; i < prog.size(); i++) {
            FormStep f = prog[i];
            if (f.op == FormStep::LEAF) { f.op = FormStep::REF; f.col = bit_of[i]; f.lo = f.hi = 0; }
            d.form[used++] = f;
        }
        d.dsrc2[k] = used - d.dsrc[k];
    }
}

// A row-id column that only CONDITIONS read (the reference's anti-join shape `k - row id` as a truth value: every row but row k)
// means the row's number in the table: on a rank of a sharded run it counts from the table's first row.  One that INDEXES a lookup
// (the bit of the row's own id in a set built over this shard's rows: co-partitioned placements) keeps counting from the shard's.
static bool rowid_counts_from_the_table(const std::vector<ScanColumn> &sc) {
    bool any = false, as_index = false;
    for (const ScanColumn &c : sc) any |= c.kind == VC_ROWID;
    for (const ScanColumn &c : sc) {
        if (c.kind == VC_DIRECT || c.kind == VC_FORM || c.kind == VC_ROWID) continue;
        for (int src : {c.idx, c.idx2}) if (src >= 0 && (size_t)src < sc.size() && sc[(size_t)src].kind == VC_ROWID) as_index = true;
    }
    return any && !as_index;
}

// Columns a scan must read with their stored values (vdl_column_image.h: the `raw_use` / `per_row_value` of the use rules): in every
// role the sources of derived columns other than formula tests -- of lookups, of differences
static uint32_t raw_value_uses(const std::vector<ScanColumn> &sc) {
    uint32_t m = 0;
    for (const ScanColumn &c : sc)
        if (c.kind != VC_DIRECT && c.kind != VC_FORM) for (int src : {c.idx, c.idx2}) if (src >= 0 && src < 32) m |= 1u << src;
    return m;
}

// the image a column's reader may use in its place: images are on, for a lookup's target lookup images too (vdl_set_lookup_images,
// under vdl_set_column_images), and the image is there -- built on the device, or declared on a context without one
static bool has_image(const vdl_ctx *c, const Column &col, bool lookup) {
    return c->images && (!lookup || c->lookup_images) && col.image.width > 0 && (col.image_buf || c->device < 0);
}

// What differs between the scan roles, for the binder
struct BindRules {
    // the role's use rule: img::use_in_aggregate (aggregate scans, global and grouped) or img::use_in_vscan (fronts, dimension and
    // semi-join scans)
    img::Use (*use)(const img::Image &, bool) = img::use_in_vscan;
    uint32_t values = 0;          // bit k: the scan needs column k with its stored value (the rule's second argument)
    int packed = 0;               // 0 = byte images only; 1 = the filter columns from their bit-packed images, 2 = every table column that has one
    bool steps = false;           // step images may be read
    // whatever is read from an image is decoded where it is loaded and keeps the plan's bounds and tests (the take side of a front:
    // base + scale * e once per survivor, at any scale -- WHICH columns are read from an image stays the use rule's answer)
    bool decode_loaded = false;
};
// ... and what the binder found beside the kernel arguments
struct Bound {
    int64_t n = -1;               // rows of the scanned table
    uint32_t encoded = 0;         // bit k: column k is read from an image and stays encoded: its tests and factors are rewritten by ims[k]
    img::Image ims[kMaxVCols];
};

// Column k of the scan: kind, bounds, derivation; for a table column (streamed) and for the target of a lookup the stored form it is
// read from -- ptr, width, pbits, the image / limage / packed / steps / decode bits, ibase / iscale, dn -- and its bounds in that
// form's domain.  A step image goes before a byte image (it decodes to the column's own values wherever it is loaded: every use is
// legal, the plan's bounds stay); a packed image overrides a byte image.
static void bind_column(vdl_ctx *c, const std::string &table, const std::vector<ScanColumn> &sc, int k, const BindRules &r, MScanCols &cols, MScanDesc &d, Bound &b) {
    const ScanColumn &s = sc[(size_t)k];
    const uint32_t bit = 1u << k;
    cols.kind[k] = bound_kind(c, sc, s);
    cols.filtered[k] = (s.lo != INT64_MIN || s.hi != INT64_MAX) ? 1 : 0;
    d.flo[k] = s.lo; d.fhi[k] = s.hi;
    d.dkind[k] = cols.kind[k]; d.dsrc[k] = s.idx; d.dsrc2[k] = s.idx2;
    const bool streamed = s.kind == VC_DIRECT;
    if (!streamed && s.kind != VC_GATHER && s.kind != VC_INRANGE) {      // VC_BITS / VC_LUT: patched in before every launch (patch_prelude); computed columns
        cols.ptr[k] = nullptr; cols.width[k] = 8;
        return;
    }
    const Column &col = find_col(c, s.name);
    if (streamed) {
        if (b.n >= 0 && col.n != b.n) throw Error(VDL_ERR_SHAPE, "columns of table '" + table + "' have different lengths in the catalog");
        b.n = col.n;
    } else {
        d.dn[k] = col.n;                                                 // a column of another table, looked up / its length
    }
    cols.ptr[k] = col.dev; cols.width[k] = col.width;
    if (streamed && r.steps && c->images && c->step_images && col.steps.present && (col.steps_buf || c->device < 0)) {
        cols.steps |= bit;
        cols.ptr[k] = col.steps_buf ? col.steps_buf->p : nullptr;
        d.ibase[k] = col.steps.base;
        // (its values are base .. base + n - 1 at most: where they fit 32 signed bits the kernels make the sum in 32)
        cols.width[k] = col.steps.base >= INT32_MIN && col.steps.base <= (int64_t)INT32_MAX - col.n ? 4 : 8;
        return;
    }
    const bool value = (r.values >> k) & 1u;
    img::Image im = col.image;
    img::Use use = (streamed || s.kind == VC_GATHER) && has_image(c, col, !streamed) ? r.use(im, value) : img::USE_CATALOG;
    if (use != img::USE_CATALOG) { cols.ptr[k] = col.image_buf ? col.image_buf->p : nullptr; cols.width[k] = im.width; }
    img::Image pim;                                                      // the packed image as an image: for the rules and compose
    pim.width = 4; pim.base = col.packed.base; pim.scale = col.packed.scale;
    const img::Use puse = streamed && r.packed && c->images && col.packed.bits && (r.packed == 2 || cols.filtered[k]) ? r.use(pim, value) : img::USE_CATALOG;
    const bool packed = puse != img::USE_CATALOG;
    if (packed) {                                                        // bounds on e' in [0, 2^bits - 1], factors composed with (base', scale)
        use = puse;
        im = pim;
        cols.packed |= bit;
        cols.pbits[k] = col.packed.bits;
        cols.ptr[k] = col.packed_buf ? col.packed_buf->p : nullptr; cols.width[k] = 4;
    }
    if (use == img::USE_CATALOG) return;
    (streamed ? cols.image : cols.limage) |= bit;
    b.ims[k] = im;
    d.ibase[k] = im.base; d.iscale[k] = im.scale;
    if (use == img::USE_DECODED || r.decode_loaded) {                    // decoded by the kernel (MsArgs::decode): the plan's bounds stay
        if (!im.pure()) cols.decode |= bit;
        return;
    }
    // left encoded: its bounds in the encoded domain (the filtered bit stays what the plan says)
    b.encoded |= bit;
    if (packed) img::map_range_packed(col.packed, s.lo, s.hi, &d.flo[k], &d.fhi[k]); else img::map_range(im, s.lo, s.hi, &d.flo[k], &d.fhi[k]);
}

// The columns of a scan as kernel arguments, every column through bind_column; then the formula columns, with the tests of the
// columns that stayed encoded rewritten into their images' domains.  (Tables of the prelude are patched in later: patch_prelude.)
static Bound bind_columns(vdl_ctx *c, const std::string &table, const std::vector<ScanColumn> &sc, const BindRules &r, MScanCols &cols, MScanDesc &d) {
    Bound b;
    cols.ncol = (int)sc.size();
    for (int k = 0; k < cols.ncol; k++) bind_column(c, table, sc, k, r, cols, d, b);
    bind_forms(sc, d);
    for (int k = 0; k < cols.ncol; k++) {
        cols.lo[k] = d.flo[k]; cols.hi[k] = d.fhi[k];
        if (cols.kind[k] != VC_FORM) continue;
        for (int f = d.dsrc[k]; f < d.dsrc[k] + d.dtests[k]; f++)
            if (d.form[f].col >= 0 && ((b.encoded >> d.form[f].col) & 1u)) img::map_range(b.ims[d.form[f].col], d.form[f].lo, d.form[f].hi, &d.form[f].lo, &d.form[f].hi);
    }
    cols.n = b.n;
    return b;
}

// ---- aggregate scans ------------------------------------------------------------------------------------------------------------
// Scan s of the fused plan (global scans first, then the grouped ones) for k_mscan and the specialised scans; the table's row count.
// A raw use admits a pure narrowing only, nothing is decoded: the factors of the columns read from images are composed with them.
int64_t bind_scan(vdl_ctx *c, const vdl_plan *p, size_t s, MScanCols &cols, MScanDesc &d, int64_t *bytes_per_row, int64_t row0, int packed) {
    const FusedPlan &F = p->fused;
    const size_t ns = F.scans.size();
    const GroupScanPlan *gp = s < ns ? nullptr : &F.gscans[s - ns];
    const std::vector<ScanColumn> &sc = scan_columns(p, s);
    const std::vector<ScanAgg> &aggs = gp ? gp->aggs : F.scans[s].aggs;
    cols = MScanCols{};
    d = MScanDesc{};
    // raw uses: sources of derived columns, loads of the group key, the column of a FIRST aggregate
    BindRules r;
    r.use = img::use_in_aggregate;
    r.packed = packed;
    r.values = raw_value_uses(sc);
    if (gp) for (const KeyStep &k : gp->key) if (k.kind == KeyStep::LOAD && k.col >= 0 && k.col < 32) r.values |= 1u << k.col;
    for (const ScanAgg &ag : aggs) if (ag.kind == AGG_FIRST) for (const ScanFactor &f : ag.fac) if (f.col >= 0 && f.col < 32) r.values |= 1u << f.col;
    const Bound b = bind_columns(c, gp ? gp->table : F.scans[s].table, sc, r, cols, d);
    *bytes_per_row = 0;
    for (int k = 0; k < cols.ncol; k++) if (cols.kind[k] == VC_DIRECT) *bytes_per_row += cols.width[k];
    cols.row0 = row0;
    cols.rowid_global = rowid_counts_from_the_table(sc);
    d.nagg = (int)aggs.size();
    for (int j = 0; j < d.nagg; j++) {
        const ScanAgg &ag = aggs[(size_t)j];
        MAggDesc &m = d.agg[j];
        m.kind = ag.kind;
        m.constant = ag.constant;
        for (const ScanFactor &f : ag.fac) {
            int64_t a = f.a, sf = f.s;
            if ((b.encoded >> f.col) & 1u) img::compose(b.ims[f.col], f.a, f.s, &a, &sf);      // a + s * (base + scale * e)
            m.used |= 1u << f.col;
            if (img::plain(a, sf)) m.plain |= 1u << f.col;
            m.fa[f.col] = a; m.fs[f.col] = sf;
        }
    }
    if (gp) {                                                            // the grouped scan's key program and pivots
        d.nkey = (int)gp->key.size();
        for (int k = 0; k < d.nkey; k++) d.key[k] = gp->key[(size_t)k];
        d.pmin = gp->pmin; d.pcount = gp->pcount;
    }
    return b.n;
}

// the single-aggregate k_scan's arguments (use_kscan: table columns only, read from the catalog); the table's row count
int64_t bind_kscan(vdl_ctx *c, const ScanPlan &sp, ScanArgs &a, int64_t *bytes_per_row) {
    a.ncol = (int)sp.cols.size(); a.nagg = 1; a.never = sp.never ? 1 : 0;
    int64_t n = -1;
    *bytes_per_row = 0;
    for (int k = 0; k < a.ncol; k++) {
        const Column &col = find_col(c, sp.cols[(size_t)k].name);
        if (n >= 0 && col.n != n) throw Error(VDL_ERR_SHAPE, "columns of table '" + sp.table + "' have different lengths in the catalog");
        n = col.n;
        a.ptr[k] = col.dev; a.width[k] = col.width;
        a.lo[k] = sp.cols[(size_t)k].lo; a.hi[k] = sp.cols[(size_t)k].hi;
        a.filtered[k] = (a.lo[k] != INT64_MIN || a.hi[k] != INT64_MAX) ? 1 : 0;
        *bytes_per_row += col.width;
    }
    a.n = n;
    const ScanAgg &ag = sp.aggs[0];
    a.kind[0] = ag.kind; a.constant[0] = ag.constant;
    for (const ScanFactor &f : ag.fac) {
        a.used[0] |= 1u << f.col;
        if (img::plain(f.a, f.s)) a.plain[0] |= 1u << f.col;
        a.fa[0][f.col] = f.a; a.fs[0][f.col] = f.s;
    }
    return n;
}

// ---- what a bound scan reads from images, for vdl_plan_image_columns / _step_columns / _lookup_columns ----------------------------
// "name:width ..." of the columns of `mask`, or "name:s ..." (a step image has no width to name)
static std::string columns_text(const std::vector<ScanColumn> &sc, const MScanCols &cols, uint32_t mask, bool step) {
    std::string t;
    for (int k = 0; k < cols.ncol && (size_t)k < sc.size(); k++)
        if ((mask >> k) & 1u) t += (t.empty() ? "" : " ") + sc[(size_t)k].name + ":" + (step ? "s" : std::to_string(cols.width[k]));
    return t;
}
void note_roles(vdl_plan *p, const std::string &role, const std::vector<ScanColumn> &sc, const MScanCols &cols, uint32_t which) {
    p->roles[role] = {columns_text(sc, cols, cols.image & which, false), columns_text(sc, cols, cols.steps & which, true), columns_text(sc, cols, cols.limage & which, false)};
}

// ---- scans with derived columns -------------------------------------------------------------------------------------------------
// A column whose values the select pass needs per row -- the sources of lookups and differences, plus `per_row`: the position of a
// semi-join -- and that is read from an image that is no pure narrowing is decoded with the tile (MsArgs::decode, one add) and keeps
// the plan's filters; every other one has its filter and formula tests rewritten into the encoded domain.
static BindRules vscan_rules(const std::vector<ScanColumn> &sc, uint32_t per_row = 0) {
    BindRules r;
    r.values = per_row | raw_value_uses(sc);
    r.steps = true;
    return r;
}

// the prelude's dimension scan or semi-join scan k -- the select pass with nothing to take: its columns, its roles and what it writes
// (the output buffer, and a semi-join's dn[index_col], belong to the run); the table's row count
int64_t bind_prelude_scan(vdl_ctx *c, vdl_plan *p, size_t k, MScanCols &cols, MScanDesc &d) {
    const PreludeItem &it = p->fused.prelude[k];
    const bool semi = it.kind == PreludeItem::SEMI_BITMAP;
    const uint32_t pos = semi && it.index_col >= 0 && it.index_col < 32 ? 1u << it.index_col : 0u;      // (the semi-join's positions)
    const int64_t n = bind_columns(c, it.table, it.cols, vscan_rules(it.cols, pos), cols, d).n;
    note_roles(p, (semi ? "semi" : "dim") + std::to_string(k), it.cols, cols);
    d.bitmap_only = semi ? 2 : 1;                                       // a dimension scan: bitmap only, no positions, no counts
    if (semi) { d.pmin = it.modulus; d.nout = 1; d.out_col[0] = it.index_col; }
    return n;
}

// hand the prelude's tables to a scan that looks them up
void patch_prelude(const vdl_plan *p, const std::vector<ScanColumn> &sc, MScanCols &cols, MScanDesc &d) {
    for (size_t k = 0; k < sc.size(); k++) {
        if (sc[k].kind != VC_BITS && sc[k].kind != VC_LUT) continue;
        const BufP &b = p->prelude_buf[(size_t)sc[k].prelude];
        cols.ptr[k] = b ? b->p : nullptr;
        d.dn[k] = p->prelude_n[(size_t)sc[k].prelude];
    }
}

void bind_front(vdl_ctx *c, vdl_plan *p, FrontBound &b) {
    const ProjPlan &J = p->fused.proj;
    MScanCols &cols = b.cols;
    MScanDesc &d = *b.d;
    b.wanted.assign(p->fused.prelude.size(), 0);
    for (const ScanColumn &sc : J.cols) if (sc.prelude >= 0) b.wanted[(size_t)sc.prelude] = 1;
    // both sides over all the columns: the select side by the use rules, the take side -- reading the same stored forms -- decodes
    // what it loads from an image, so its filters and formula tests are the plan's
    BindRules rules = vscan_rules(J.cols);
    MScanCols all;
    auto alld = std::make_unique<MScanDesc>();
    bind_columns(c, J.table, J.cols, rules, all, *alld);
    rules.decode_loaded = true;
    b.n = bind_columns(c, J.table, J.cols, rules, cols, d).n;
    cols.row0 = b.scols.row0 = p->row_offset;
    cols.rowid_global = b.scols.rowid_global = p->front_rowid_global || rowid_counts_from_the_table(J.cols);      // (the sharded front route: every row id is the table's)
    // columns that decide a row's survival: the filtered ones and what they are derived from; a lookup whose range check is
    // done by another deciding column through the same index (the dimension bitmap, an INRANGE) decides nothing itself.
    // Everything else is read for the surviving rows only, in the write pass.
    {
        std::vector<char> decides((size_t)cols.ncol, 0);
        for (int k = 0; k < cols.ncol; k++) decides[(size_t)k] = cols.filtered[k] || J.cols[(size_t)k].kind == VC_INRANGE;
        for (int k = 0; k < cols.ncol; k++) {
            const ScanColumn &sc = J.cols[(size_t)k];
            if (sc.kind != VC_GATHER || decides[(size_t)k]) continue;
            bool checked = false;
            for (int j = 0; j < cols.ncol; j++) {
                const ScanColumn &o = J.cols[(size_t)j];
                checked |= j != k && o.idx == sc.idx && (o.kind == VC_INRANGE || o.kind == VC_BITS || (o.kind == VC_GATHER && decides[(size_t)j] && j < k));
            }
            if (!checked) decides[(size_t)k] = 1;                     // its own range check can drop the row
        }
        for (int k = cols.ncol - 1; k >= 0; k--) {
            if (!decides[(size_t)k]) continue;
            for (int src : J.cols[(size_t)k].sources()) decides[(size_t)src] = 1;
        }
        for (int k = 0; k < cols.ncol; k++) cols.lazy[k] = decides[(size_t)k] ? 0 : 1;
    }
    // the select pass: deciding columns only, renumbered (its register use grows with the column count)
    MScanCols &scols = b.scols;
    MScanDesc *sdesc = b.sdesc.get();
    const MScanDesc &ad = *alld;
    b.renum.assign((size_t)cols.ncol, -1);
    std::vector<int> &renum = b.renum;
    for (int k = 0; k < cols.ncol; k++) {
        if (cols.lazy[k]) continue;
        const int j = scols.ncol++;
        renum[(size_t)k] = j;
        scols.ptr[j] = all.ptr[k]; scols.width[j] = all.width[k]; scols.filtered[j] = all.filtered[k];
        scols.lo[j] = all.lo[k]; scols.hi[j] = all.hi[k]; scols.kind[j] = all.kind[k];
        sdesc->flo[j] = ad.flo[k]; sdesc->fhi[j] = ad.fhi[k]; sdesc->dkind[j] = ad.dkind[k]; sdesc->dn[j] = ad.dn[k]; sdesc->dtests[j] = ad.dtests[k];
        scols.image |= ((all.image >> k) & 1u) << j; scols.decode |= ((all.decode >> k) & 1u) << j; scols.steps |= ((all.steps >> k) & 1u) << j;
        scols.limage |= ((all.limage >> k) & 1u) << j;
        sdesc->ibase[j] = ad.ibase[k]; sdesc->iscale[j] = ad.iscale[k];
        if (ad.dkind[k] == VC_FORM) {                         // its steps stay where they are in the pool; the tests' columns are
            sdesc->dsrc[j] = ad.dsrc[k]; sdesc->dsrc2[j] = ad.dsrc2[k];      // renumbered (monotonic: they stay sorted by column)
            for (int f = ad.dsrc[k]; f < ad.dsrc[k] + ad.dsrc2[k]; f++) {
                sdesc->form[f] = ad.form[f];
                if (ad.form[f].op == FormStep::LEAF) sdesc->form[f].col = renum[(size_t)ad.form[f].col];
            }
            continue;
        }
        sdesc->dsrc[j] = ad.dsrc[k] >= 0 ? renum[(size_t)ad.dsrc[k]] : -1;
        sdesc->dsrc2[j] = ad.dsrc2[k] >= 0 ? renum[(size_t)ad.dsrc2[k]] : -1;
    }
    scols.n = b.n;
    // the take pass: one packed vector per produced column (statements that are the same column share it), and what those
    // columns are derived from
    // (`distinct` holds output codes: a column, or -2 - e for the row expression e the pass evaluates: ProjPlan::exprs)
    for (int oc : J.node_col) if (oc != -1 && std::find(b.distinct.begin(), b.distinct.end(), oc) == b.distinct.end()) b.distinct.push_back(oc);
    d.nout = (int)b.distinct.size();
    d.take = 0;
    d.nexpr = (int)J.exprs.size();
    d.nkey = 0;
    for (size_t e = 0; e < J.exprs.size(); e++) {
        d.expr_at[e] = d.nkey; d.expr_len[e] = (int)J.exprs[e].size();
        for (const KeyStep &st : J.exprs[e]) {
            if (d.nkey >= kMaxKeySteps) throw Error(VDL_ERR_UNSUPPORTED, "internal: the front's expressions exceed the descriptor's step pool");
            d.key[d.nkey++] = st;
            if (st.kind == KeyStep::LOAD) d.take |= 1u << st.col;
        }
    }
    for (size_t o = 0; o < b.distinct.size(); o++) { d.out_col[o] = b.distinct[o]; if (b.distinct[o] >= 0) d.take |= 1u << b.distinct[o]; }
    for (int k = cols.ncol - 1; k >= 0; k--) {
        if (!((d.take >> k) & 1u)) continue;
        for (int src : J.cols[(size_t)k].sources()) d.take |= 1u << src;
    }
    // table columns both sides of the front read (they decide survival AND the outputs need them: the join index of a fact table whose
    // dimension is filtered) stay in LDS for the survivors (MScanDesc::carry)
    d.carry = 0; sdesc->carry = 0;
    int taken = 0;
    for (int k = 0; k < cols.ncol && taken < kMaxCarry; k++) {
        if (cols.lazy[k] || cols.kind[k] != VC_DIRECT || !((d.take >> k) & 1u) || renum[(size_t)k] < 0) continue;
        if (((cols.decode & ~all.decode) >> k) & 1u) continue;       // the select side holds its encoded values: the take side loads it
        d.carry |= 1u << k;
        sdesc->carry |= 1u << renum[(size_t)k];
        taken++;
    }
    uint32_t deciding = 0;
    for (int k = 0; k < cols.ncol; k++) if (renum[(size_t)k] >= 0) deciding |= 1u << k;
    note_roles(p, "front.select", J.cols, cols, deciding);
    note_roles(p, "front.take", J.cols, cols, d.take);
}
// the prelude's tables of this run, in both passes' arguments
void patch_front(const vdl_plan *p, FrontBound &b) {
    patch_prelude(p, p->fused.proj.cols, b.cols, *b.d);
    for (int k = 0; k < b.cols.ncol; k++) {
        if (b.renum[(size_t)k] < 0) continue;
        b.scols.ptr[b.renum[(size_t)k]] = b.cols.ptr[k];
        b.sdesc->dn[b.renum[(size_t)k]] = b.d->dn[k];
    }
}

}  // namespace eng
}  // namespace vdl
