// vdl_jit.cpp -- a fused scan specialised for ONE plan at run time.
//
// The precompiled scan kernels (vdl_mscan.hip) interpret a descriptor: which columns are lookups, which carry filters, the
// group key's steps, every aggregate's factors, the conditions' tests.  That costs vector instructions per row -- selects
// over all columns to find a source column, dispatch on kinds -- and a 28 B/row scan at 8 TB/s has only about 140 of them
// per row slice of a wave.  Here the SAME device code (vdl_mscan_body.h, embedded as text at build time) is compiled by
// hiprtc with the plan's descriptor as a compile-time constant: every descriptor-driven branch and loop folds away and
// what is left is the straight-line code of this query.  (The text this engine executes "is meant to be executed by a voodoo
// implementation", /root/reference/README.md:57 -- the system of the cited paper, which generates kernels per program.)
// One hiprtc compile per distinct (descriptor, shape) per process -- seconds -- cached in memory and, when VDL_JIT_CACHE names a directory, on disk.  Opt-in: vdl_plan_set_jit / VDL_JIT=1; a plan
// whose specialisation fails to build runs on the precompiled kernels and says so in its description.
#include "vdl_jit.h"

#include <dlfcn.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <mutex>
#include <sstream>

namespace vdl {
namespace jit {

namespace {

#ifndef VDL_PROJ_U
#define VDL_PROJ_U 4
#endif
constexpr int VDL_PROJ_U_HOST = VDL_PROJ_U;
#ifndef VDL_FRONT_BATCH
#define VDL_FRONT_BATCH 4
#endif
constexpr int VDL_FRONT_BATCH_HOST = VDL_FRONT_BATCH;      // (tiles per batch of the one-pass front as this library was built: the launcher's grid and look-back area follow it)
const char kEmbedded[] =
#include "vdl_jit_src.inc"
    ;

// ---- hiprtc, bound at first use ------------------------------------------------------------------------------------------
struct Rtc {
    void *lib = nullptr;
    int (*create)(void **, const char *, const char *, int, const char **, const char **) = nullptr;
    int (*compile)(void *, int, const char **) = nullptr;
    int (*log_size)(void *, size_t *) = nullptr;
    int (*log)(void *, char *) = nullptr;
    int (*code_size)(void *, size_t *) = nullptr;
    int (*code)(void *, char *) = nullptr;
    int (*destroy)(void **) = nullptr;
    int (*version)(int *, int *) = nullptr;      // optional
    std::string why;
};
Rtc &rtc() {
    static Rtc r;
    static std::once_flag once;
    std::call_once(once, [] {
        const char *names[] = {"libhiprtc.so.7", "libhiprtc.so", "/opt/rocm/lib/libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"};
        if (const char *forced = getenv("VDL_HIPRTC_LIB")) r.lib = dlopen(forced, RTLD_NOW | RTLD_LOCAL);      // (this one or none)
        else for (const char *n : names) if ((r.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
        if (!r.lib) { r.why = "libhiprtc not found"; return; }
        auto sym = [&](const char *n) { void *p = dlsym(r.lib, n); if (!p) r.why = std::string("libhiprtc lacks ") + n; return p; };
        r.create = (decltype(r.create))sym("hiprtcCreateProgram");
        r.compile = (decltype(r.compile))sym("hiprtcCompileProgram");
        r.log_size = (decltype(r.log_size))sym("hiprtcGetProgramLogSize");
        r.log = (decltype(r.log))sym("hiprtcGetProgramLog");
        r.code_size = (decltype(r.code_size))sym("hiprtcGetCodeSize");
        r.code = (decltype(r.code))sym("hiprtcGetCode");
        r.destroy = (decltype(r.destroy))sym("hiprtcDestroyProgram");
        r.version = (decltype(r.version))dlsym(r.lib, "hiprtcVersion");
    });
    return r;
}

std::string lit(int64_t v) {
    if (v == INT64_MIN) return "(-9223372036854775807LL - 1)";
    return std::to_string(v) + "LL";
}

uint64_t fnv(const std::string &s) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (unsigned char ch : s) h = (h ^ ch) * 0x100000001B3ull;
    return h;
}

// a second, unrelated 64-bit hash of the source: a cache entry must match both (and the length) before its code is loaded
uint64_t mix64(const std::string &s) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (unsigned char ch : s) {
        h += ch + 0x9E3779B97F4A7C15ull;
        h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
        h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
        h ^= h >> 31;
    }
    return h;
}

std::mutex g_mu;
std::map<std::string, std::vector<char>> g_code;        // key (hash + arch) -> code object, per process

// ---- the on-disk cache ---------------------------------------------------------------------------------------------------
// Code objects are device code that runs against this process's GPU memory, so a cache entry is only ever read from a
// directory that belongs to the caller and that nobody else can write: the directory (created 0700, parents included when
// missing) must be a real directory -- not a symbolic link -- owned by the effective user and closed to group and others;
// entries are regular files of the same owner opened with O_NOFOLLOW, and carry a header {magic, both hashes and the length
// of the source they were built from, code length} that must match the source about to be compiled.  The key holds the
// hiprtc version, so a toolchain upgrade does not meet stale code.  Anything that does not check out is ignored (and said on
// stderr once): the scan is compiled again, never loaded from there.
struct CacheHeader { char magic[8]; uint64_t h1, h2, src_len, code_len; };
const char kCacheMagic[8] = {'V', 'D', 'L', 'J', 'I', 'T', '2', 0};

bool make_private_dirs(const std::string &dir) {
    struct stat st;
    if (lstat(dir.c_str(), &st) == 0) return true;
    const size_t cut = dir.find_last_of('/');
    if (cut != std::string::npos && cut > 0 && !make_private_dirs(dir.substr(0, cut))) return false;
    return mkdir(dir.c_str(), 0700) == 0 || errno == EEXIST;
}
// "" when the directory cannot be trusted (why: on stderr, once per directory)
std::string trusted_cache_dir() {
    const char *dir = getenv("VDL_JIT_CACHE");
    if (!dir || !*dir) return "";
    static std::mutex mu;
    static std::map<std::string, bool> verdicts;
    std::lock_guard<std::mutex> g(mu);
    auto it = verdicts.find(dir);
    if (it != verdicts.end()) return it->second ? dir : "";
    std::string why;
    struct stat st;
    if (!make_private_dirs(dir)) why = "cannot be created";
    else if (lstat(dir, &st) != 0) why = "cannot be examined";
    else if (!S_ISDIR(st.st_mode)) why = "is not a directory (symbolic links are not followed)";
    else if (st.st_uid != geteuid()) why = "belongs to another user";
    else if (st.st_mode & (S_IWGRP | S_IWOTH)) why = "is writable by group or others";
    verdicts[dir] = why.empty();
    if (!why.empty()) fprintf(stderr, "vdl: VDL_JIT_CACHE=%s %s: not used, specialised scans are compiled in this process\n", dir, why.c_str());
    return why.empty() ? dir : "";
}
bool cache_read(const std::string &path, const std::string &src, std::vector<char> &code) {
    const int fd = open(path.c_str(), O_RDONLY | O_NOFOLLOW | O_CLOEXEC);
    if (fd < 0) return false;
    bool ok = false;
    struct stat st;
    CacheHeader h;
    if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_uid == geteuid() && !(st.st_mode & (S_IWGRP | S_IWOTH)) &&
        read(fd, &h, sizeof h) == (ssize_t)sizeof h && memcmp(h.magic, kCacheMagic, 8) == 0 && h.h1 == fnv(src) && h.h2 == mix64(src) &&
        h.src_len == src.size() && h.code_len > 0 && (off_t)(sizeof h + h.code_len) == st.st_size) {
        code.resize(h.code_len);
        size_t got = 0;
        while (got < code.size()) {
            const ssize_t k = read(fd, code.data() + got, code.size() - got);
            if (k <= 0) break;
            got += (size_t)k;
        }
        ok = got == code.size();
    }
    close(fd);
    if (!ok) code.clear();
    return ok;
}
void cache_write(const std::string &path, const std::string &src, const std::vector<char> &code) {
    const std::string tmp = path + ".tmp" + std::to_string((long)getpid());
    const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW | O_CLOEXEC, 0600);
    if (fd < 0) return;
    CacheHeader h;
    memcpy(h.magic, kCacheMagic, 8);
    h.h1 = fnv(src); h.h2 = mix64(src); h.src_len = src.size(); h.code_len = code.size();
    bool ok = write(fd, &h, sizeof h) == (ssize_t)sizeof h;
    size_t put = 0;
    while (ok && put < code.size()) {
        const ssize_t k = write(fd, code.data() + put, code.size() - put);
        if (k <= 0) ok = false; else put += (size_t)k;
    }
    ok = (close(fd) == 0) && ok;
    if (ok) ok = rename(tmp.c_str(), path.c_str()) == 0;
    if (!ok) unlink(tmp.c_str());
}

// VDL_JIT_BRANCHY_LATE=1 (A/B profiles): the staged forms' masked late loads as branches around plain loads, as before buffer loads
bool branchy_late() {
    const char *e = getenv("VDL_JIT_BRANCHY_LATE");
    return e && atoi(e) != 0;
}

// ---- run-time bounds (Shape::rt_bounds) -----------------------------------------------------------------------------------
// The generated text then holds the SHAPE of every range -- which sides are open, whether it is a point -- and no value: the
// kernel reads the values from the launch's descriptor (vdl_mscan_body.h range_bounds), and plans that differ in their literals
// alone yield one source, one cache entry, one kernel.  A side is open when its bound lies at or beyond the end of the domain the
// column's values are read in: then no stored value fails it and the compare folds away as it does with the literal.
struct Domain { int64_t lo = INT64_MIN, hi = INT64_MAX; };
// what v[c] can hold: a packed image's 0 .. 2^bits - 1, a table column's or byte image's signed range at its width; anything for a
// derived column and for a column decoded with the tile
Domain column_domain(const MsArgs &C, int c) {
    Domain d;
    if (c < 0 || c >= C.ncol || (((C.derived | C.decode) >> c) & 1u)) return d;
    if ((C.packed >> c) & 1u) { d.lo = 0; d.hi = C.bits(c) >= 63 ? INT64_MAX : ((int64_t)1 << C.bits(c)) - 1; return d; }
    const int w = C.width(c);
    if (w < 8) { d.lo = -((int64_t)1 << (8 * w - 1)); d.hi = ((int64_t)1 << (8 * w - 1)) - 1; }
    return d;
}
struct RangeShape {
    bool lo_open = false, hi_open = false, point = false;
    // as the descriptor's constants (range_bounds): INT64_MIN / INT64_MAX: open; (0, 0): a point; (0, 1): both bounds are read
    int64_t clo() const { return lo_open ? INT64_MIN : 0; }
    int64_t chi() const { return hi_open ? INT64_MAX : point ? 0 : 1; }
};
RangeShape range_shape(const Domain &dom, int64_t lo, int64_t hi) {
    RangeShape s;
    s.lo_open = lo <= dom.lo;
    s.hi_open = hi >= dom.hi;
    s.point = !s.lo_open && !s.hi_open && lo == hi;
    return s;
}
// "alive[r] & <tests of v[c][r] against the launch's bounds>" for one filter column of a generated stage line; `u32`: the
// packed form's 32-bit unsigned compares
std::string rt_filter_line(const MsArgs &C, const MScanDesc &D, int c, bool u32) {
    const RangeShape s = range_shape(column_domain(C, c), D.flo[c], D.fhi[c]);
    if (s.lo_open && s.hi_open) return "";
    const std::string v = std::string(u32 ? "(uint32_t)" : "") + "v[" + std::to_string(c) + "][r]";
    const std::string lo = std::string(u32 ? "(uint32_t)" : "") + "Dr.flo[" + std::to_string(c) + "]", hi = std::string(u32 ? "(uint32_t)" : "") + "Dr.fhi[" + std::to_string(c) + "]";
    std::string t = " _Pragma(\"unroll\") for (int r = 0; r < RW; r++) alive[r] = alive[r]";
    if (s.point) t += " & (" + v + " == " + lo + ")";
    else {
        if (!s.lo_open) t += " & (" + v + " >= " + lo + ")";
        if (!s.hi_open) t += " & (" + v + " <= " + hi + ")";
    }
    return t + ";";
}

std::atomic<int64_t> g_compiled{0}, g_from_disk{0}, g_from_memory{0};

}  // namespace

void counters(int64_t *compiled, int64_t *from_disk, int64_t *from_memory) {
    if (compiled) *compiled = g_compiled.load();
    if (from_disk) *from_disk = g_from_disk.load();
    if (from_memory) *from_memory = g_from_memory.load();
}

// the descriptor as constexpr functions: only what differs from the defaults is written
// (rt: run-time bounds -- the ranges' shapes in place of their values)
static std::string desc_text(Kind kind, const MsArgs &C, const MScanDesc &D, const char *suffix = "", bool rt = false) {
    auto lo_of = [&](int col, int64_t lo, int64_t hi) { return rt ? range_shape(column_domain(C, col), lo, hi).clo() : lo; };
    auto hi_of = [&](int col, int64_t lo, int64_t hi) { return rt ? range_shape(column_domain(C, col), lo, hi).chi() : hi; };
    std::ostringstream o;
    o << "namespace vdl {\n";
    o << "constexpr MsArgs jit_args" << suffix << "() {\n    MsArgs a{};\n";
    o << "    a.ncol = " << C.ncol << "; a.widths = " << C.widths << "ull; a.filtered = " << C.filtered << "u; a.derived = " << C.derived
      << "u; a.lazy = " << C.lazy << "u; a.stages = " << C.stages << "ull; a.queued = " << C.queued << "; a.decode = " << C.decode << "u;\n";
    if (C.packed) o << "    a.packed = " << C.packed << "u; a.pbits = " << C.pbits << "ull;\n";
    if (C.steps) o << "    a.steps = " << C.steps << "u;\n";
    o << "    return a;\n}\n";
    o << "constexpr MScanDesc jit_desc" << suffix << "() {\n    MScanDesc d{};\n";
    o << "    d.nagg = " << D.nagg << "; d.nkey = " << D.nkey << "; d.replicas = " << D.replicas << "; d.pmin = " << lit(D.pmin) << "; d.pcount = " << lit(D.pcount) << ";\n";
    int pool = 0;
    for (int k = 0; k < C.ncol; k++) {
        if ((C.filtered >> k) & 1u) o << "    d.flo[" << k << "] = " << lit(lo_of(k, D.flo[k], D.fhi[k])) << "; d.fhi[" << k << "] = " << lit(hi_of(k, D.flo[k], D.fhi[k])) << ";\n";
        if ((C.decode >> k) & 1u) o << "    d.ibase[" << k << "] = " << lit(D.ibase[k]) << "; d.iscale[" << k << "] = " << lit(D.iscale[k]) << ";\n";
        if ((C.steps >> k) & 1u) o << "    d.ibase[" << k << "] = " << lit(D.ibase[k]) << ";\n";      // (a step image's base)
        if ((C.derived >> k) & 1u) {
            o << "    d.dkind[" << k << "] = " << D.dkind[k] << "; d.dsrc[" << k << "] = " << D.dsrc[k] << "; d.dsrc2[" << k << "] = " << D.dsrc2[k]
              << "; d.dtests[" << k << "] = " << D.dtests[k] << ";\n";
            if (D.dkind[k] == VC_FORM) pool = std::max(pool, D.dsrc[k] + D.dsrc2[k]);
        }
    }
    for (int f = 0; f < pool; f++)
        o << "    d.form[" << f << "].op = " << D.form[f].op << "; d.form[" << f << "].col = " << D.form[f].col << "; d.form[" << f << "].lo = "
          << lit(D.form[f].op == FormStep::LEAF ? lo_of(D.form[f].col, D.form[f].lo, D.form[f].hi) : D.form[f].lo) << "; d.form[" << f << "].hi = "
          << lit(D.form[f].op == FormStep::LEAF ? hi_of(D.form[f].col, D.form[f].lo, D.form[f].hi) : D.form[f].hi) << ";\n";
    o << "    d.ncomp = " << D.ncomp << "; d.key_masked = " << D.key_masked << "; d.key_mask = " << lit(D.key_mask) << ";\n";
    for (int k = 0; k < D.ncomp; k++)
        o << "    d.comp[" << k << "].col = " << D.comp[k].col << "; d.comp[" << k << "].rsh = " << D.comp[k].rsh << "; d.comp[" << k << "].lsh = " << D.comp[k].lsh
          << "; d.comp[" << k << "].sub = " << lit(D.comp[k].sub) << ";\n";
    for (int s = 0; s < D.nkey; s++)
        o << "    d.key[" << s << "].kind = (KeyStep::Kind)" << (int)D.key[s].kind << "; d.key[" << s << "].target = " << D.key[s].target << "; d.key[" << s << "].col = "
          << D.key[s].col << "; d.key[" << s << "].bin = " << D.key[s].bin << "; d.key[" << s << "].const_left = " << D.key[s].const_left << "; d.key[" << s
          << "].k = " << lit(D.key[s].k) << ";\n";
    for (int j = 0; j < D.nagg; j++) {
        const MAggDesc &a = D.agg[j];
        o << "    d.agg[" << j << "].kind = " << a.kind << "; d.agg[" << j << "].used = " << a.used << "u; d.agg[" << j << "].plain = " << a.plain << "u; d.agg[" << j
          << "].constant = " << lit(a.constant) << ";\n";
        for (int k = 0; k < C.ncol; k++)
            if ((a.used >> k) & 1u) o << "    d.agg[" << j << "].fa[" << k << "] = " << lit(a.fa[k]) << "; d.agg[" << j << "].fs[" << k << "] = " << lit(a.fs[k]) << ";\n";
    }
    if (kind != MSCAN) {
        o << "    d.take = " << D.take << "u; d.nout = " << D.nout << "; d.bitmap_only = " << D.bitmap_only << "; d.carry = " << D.carry << "u;\n";
        for (int k = 0; k < D.nout; k++) o << "    d.out_col[" << k << "] = " << D.out_col[k] << ";\n";
        o << "    d.nexpr = " << D.nexpr << ";\n";
        for (int k = 0; k < D.nexpr; k++) o << "    d.expr_at[" << k << "] = " << D.expr_at[k] << "; d.expr_len[" << k << "] = " << D.expr_len[k] << ";\n";
    }
    o << "    return d;\n}\n}  // namespace vdl\n";
    return o.str();
}

// a column the binder made a saturated difference (VC_SUBS): the unit then compiles that branch of the embedded code in
static bool has_sat_diff(const MsArgs &C, const MScanDesc &D) {
    for (int k = 0; k < C.ncol; k++) if (D.dkind[k] == VC_SUBS) return true;
    return false;
}

// a lookup that reads the image of its target column and is decoded after the lookup (MsArgs::decode among the derived columns): the
// unit then compiles that step of the embedded code in (VDL_LOOKUP_DECODE); every other unit is the code it was
static bool has_lookup_decode(const MsArgs &C) { return (C.decode & C.derived) != 0; }

std::string scan_source(Kind kind, const MsArgs &C, const MScanDesc &D, const Shape &sh) {
    std::ostringstream o;
    o << "#define VDL_SPEC_UNROLL _Pragma(\"unroll\")\n";
    const bool rt = sh.rt_bounds;
    if (rt) o << "#define VDL_RT_BOUNDS 1\n";
    if (has_sat_diff(C, D)) o << "#define VDL_SAT_DIFF 1\n";
    if (has_lookup_decode(C)) o << "#define VDL_LOOKUP_DECODE 1\n";
    if (kind == MSCAN && sh.batch) o << "#define VDL_BATCH " << sh.batch << "\n#define VDL_BATCH_NAGG " << D.nagg << "\n";
    if (kind == MSCAN && sh.wide) o << "#define VDL_WIDE 1\n";
    if (kind == MSCAN && sh.census) o << "#define VDL_CENSUS 1\n";
    if (kind == MSCAN && C.packed) o << "#define VDL_PACKED 1\n";
    if (kind == MSCAN && C.lazy && C.packed) {
        // the packed form (vdl_mscan_body.h VDL_PACKED): the filters of the packed columns as 32-bit unsigned compares on e', then the
        // late columns from their byte images, one row per lane through a buffer resource over the stripe (a lane's rows are 64 apart:
        // no pairs).  Census builds: the wave's lanes hold consecutive rows (stride w), so a lane is the first asker of its 128-byte
        // line when no lower live lane lies in the same line.
        auto ulit = [](int64_t x) { return std::to_string((uint64_t)x & 0xffffffffull) + "u"; };
        o << "#define VDL_STAGED_PRE";
        for (int c = 0; c < C.ncol; c++) {
            if (!((C.filtered >> c) & 1u) || ((C.lazy >> c) & 1u)) continue;
            if (rt) o << rt_filter_line(C, D, c, (C.packed >> c) & 1u);
            else if ((C.packed >> c) & 1u)
                o << " _Pragma(\"unroll\") for (int r = 0; r < RW; r++) alive[r] = alive[r] & ((uint32_t)v[" << c << "][r] >= " << ulit(D.flo[c]) << ") & ((uint32_t)v[" << c
                  << "][r] <= " << ulit(D.fhi[c]) << ");";
            else          // (a filter column without a packed image: its byte image, read with the stripe)
                o << " _Pragma(\"unroll\") for (int r = 0; r < RW; r++) alive[r] = alive[r] & (v[" << c << "][r] >= " << lit(D.flo[c]) << ") & (v[" << c << "][r] <= "
                  << lit(D.fhi[c]) << ");";
        }
        o << "\n#define VDL_STAGED_POST";
        for (int c = 0; c < C.ncol; c++) {
            if (!((C.lazy >> c) & 1u)) continue;
            const int w = C.width(c);
            o << " { const __amdgpu_buffer_rsrc_t rs_ = buf_rsrc((const char *)Cr.ptr[" << c << "] + tile0 * " << w << ", (uint32_t)(tile_rows * " << w
              << ")); _Pragma(\"unroll\") for (int r = 0; r < RW; r++) {";
            if (sh.census)
                o << " { const uint64_t m_ = __ballot(pass[r]); const uint64_t a_ = (uint64_t)Cr.ptr[" << c << "] + (uint64_t)(rowid[r] - Cr.row0) * " << w << "ull;"
                  << " const int ln_ = (int)(threadIdx.x & 63u); int lo_ = ln_ - (int)((a_ & 127ull) / " << w << "ull); if (lo_ < 0) lo_ = 0;"
                  << " const bool first_ = pass[r] && ((m_ >> lo_) & ((1ull << (ln_ - lo_)) - 1ull)) == 0ull;"
                  << " const uint64_t f_ = __ballot(first_); if (ln_ == 0) census_cnt[" << c << "] += (unsigned long long)__popcll(f_); }";
            o << " v[" << c << "][r] = buf_load_one<" << w << ">(rs_, pass[r], (uint32_t)(rowid[r] - Cr.row0 - tile0) * " << w << "u); } }";
        }
        o << "\n";
    } else if (kind == MSCAN && C.lazy && C.queued) {
        // the queue form: only the filters of the columns that come with the tile, as straight-line code over the tile's rows
        o << "#define VDL_QUEUE_FILTER";
        for (int c = 0; c < C.ncol; c++)
            if (!((C.derived >> c) & 1u) && !((C.lazy >> c) & 1u) && ((C.filtered >> c) & 1u) && rt) o << rt_filter_line(C, D, c, false);
            else if (!((C.derived >> c) & 1u) && !((C.lazy >> c) & 1u) && ((C.filtered >> c) & 1u))
                o << " _Pragma(\"unroll\") for (int r = 0; r < RW; r++) alive[r] = alive[r] & (v[" << c << "][r] >= " << lit(D.flo[c]) << ") & (v[" << c << "][r] <= " << lit(D.fhi[c]) << ");";
        o << "\n";
    } else if (kind == MSCAN && C.lazy) {
        // the stages of a scan that reads late (MsArgs::stages), as straight-line code inside the body's row loop context
        // a lane's rows come in adjacent pairs (2u, 2u + 1): with aligned columns a pair of which a row is still in is ONE
        // 16-byte (int64) / 8-byte (int32) / 4-byte (int16) / 2-byte (int8: the narrow images of vdl_column_image.h) load instead
        // of two masked scalar ones; the one-row tail and unaligned columns take the scalar form
        const bool pairs = sh.vec && !getenv("VDL_JIT_NO_PAIR_LOADS");
        // census builds: the wave's lanes hold consecutive addresses (stride 2 w), so a lane is the first asker of its line when no
        // lower active lane lies in the same 128 bytes -- the lanes [lane - (a % 128) / (2 w), lane)
        auto census = [&](int c, int w, const char *on) {
            std::ostringstream l;
            if (!sh.census) return std::string();
            l << " { const uint64_t m_ = __ballot(" << on << "); const uint64_t a_ = (uint64_t)Cr.ptr[" << c << "] + (uint64_t)(rowid[r] - Cr.row0) * " << w << "ull;"
              << " const int ln_ = (int)(threadIdx.x & 63u); int lo_ = ln_ - (int)((a_ & 127ull) / " << 2 * w << "ull); if (lo_ < 0) lo_ = 0;"
              << " const bool first_ = (" << on << ") && ((m_ >> lo_) & ((1ull << (ln_ - lo_)) - 1ull)) == 0ull;"
              << " const uint64_t f_ = __ballot(first_); if (ln_ == 0) census_cnt[" << c << "] += (unsigned long long)__popcll(f_); }";
            return l.str();
        };
        // (VDL_JIT_BRANCHY_LATE=1: the masked loads as branches, the form before buffer loads -- for profiles that compare the two)
        const bool branchy = branchy_late();
        auto load = [&](int c, const char *mask) {
            std::ostringstream l;
            const int w = C.width(c);
            if (pairs && !branchy) {
                // one buffer resource per column over the rows of the lane's tile (built from wave-uniform values: tile0, tile_rows);
                // a pair of which no row is in passes an offset past it and asks memory for nothing -- no branch, so a row slice's
                // late loads go out together (vdl_mscan_body.h buf_load_pair).  The partial tile's last row has no partner: the
                // scalar form reads it (rows_left is a constant in full tiles, where that code folds away).
                l << " if (RW % 2 == 0) { const __amdgpu_buffer_rsrc_t rs_ = buf_rsrc((const char *)Cr.ptr[" << c << "] + tile0 * " << w << ", (uint32_t)(tile_rows * " << w
                  << ")); _Pragma(\"unroll\") for (int r = 0; r < RW; r += 2) { const int r1 = r + 1 < RW ? r + 1 : r;" << census(c, w, (std::string(mask) + "[r] | " + mask + "[r1]").c_str())
                  << " const bool two_ = (int64_t)((r >> 1) * (kMsBlock * 2)) + 1 < rows_left; buf_load_pair<" << w << ">(rs_, (" << mask << "[r] | " << mask
                  << "[r1]) & two_, (uint32_t)(rowid[r] - Cr.row0 - tile0) * " << w << "u, v[" << c << "][r], v[" << c << "][r1]); if (!two_ && " << mask << "[r]) v[" << c
                  << "][r] = load_scalar(Cr.ptr[" << c << "], " << w << ", rowid[r] - Cr.row0); } } else {";
            } else if (pairs) {
                const char *vt = w == 8 ? "ll2" : w == 4 ? "i32x2" : w == 2 ? "i16x2" : "i8x2";
                l << " if (RW % 2 == 0) { _Pragma(\"unroll\") for (int r = 0; r < RW; r += 2) { const int r1 = r + 1 < RW ? r + 1 : r; v[" << c << "][r] = 0; v[" << c
                  << "][r1] = 0;" << census(c, w, (std::string(mask) + "[r] | " + mask + "[r1]").c_str()) << " if (" << mask << "[r] | " << mask << "[r1]) { const int64_t i0 = rowid[r] - Cr.row0; if (i0 + 1 < Cr.n) { const " << vt << " x = *(const " << vt
                  << " *)((const char *)Cr.ptr[" << c << "] + i0 * " << w << "); v[" << c << "][r] = x.x; v[" << c << "][r1] = x.y; } else if (" << mask << "[r]) v[" << c
                  << "][r] = load_scalar(Cr.ptr[" << c << "], " << w << ", i0); } } } else {";   /* (the table's last row has no partner) */
            }
            l << " _Pragma(\"unroll\") for (int r = 0; r < RW; r++) { v[" << c << "][r] = 0; if (" << mask << "[r]) v[" << c << "][r] = load_scalar(Cr.ptr[" << c << "], "
              << w << ", rowid[r] - Cr.row0); }";
            if (pairs) l << " }";
            return l.str();
        };
        o << "#define VDL_STAGED_PRE";
        for (int st = 0; st <= 3; st++)
            for (int c = 0; c < C.ncol; c++) {
                if (((C.derived >> c) & 1u) || C.stage(c) != st) continue;
                if (st > 0) o << load(c, "alive");
                if (((C.filtered >> c) & 1u) && rt) o << rt_filter_line(C, D, c, false);
                else if ((C.filtered >> c) & 1u)
                    o << " _Pragma(\"unroll\") for (int r = 0; r < RW; r++) alive[r] = alive[r] & (v[" << c << "][r] >= " << lit(D.flo[c]) << ") & (v[" << c << "][r] <= "
                      << lit(D.fhi[c]) << ");";
            }
        for (int c = 0; c < C.ncol; c++) if (!((C.derived >> c) & 1u) && C.stage(c) == 14) o << load(c, "alive");
        o << "\n#define VDL_STAGED_POST";
        for (int c = 0; c < C.ncol; c++) if (!((C.derived >> c) & 1u) && C.stage(c) == 15) o << load(c, "pass");
        o << "\n";
    }
    o << "#define VDL_PROJ_U " << VDL_PROJ_U_HOST << "\n" << kEmbedded << "\n" << desc_text(kind, C, D, "", rt);      // (the tile of the projection scan as this library was built)
    const char *b = sh.vec ? "true" : "false";
    if (kind == MSCAN && sh.batch)
        o << "extern \"C\" __global__ __launch_bounds__(256) void " << entry_name(kind, C, D, sh) << "(const vdl::MsArgs Cr, const vdl::MsBatch B) {\n"
             "    constexpr vdl::MsArgs C = vdl::jit_args();\n"
             "    constexpr vdl::MScanDesc D = vdl::jit_desc();\n"
             "    vdl::mscan_body<" << sh.nc << ", " << sh.u << ", " << b << ", " << b << ", " << (sh.grouped ? "true" : "false") << ", " << (sh.der ? "true" : "false")
          << ", false>(C, Cr, D, *B.d[0], B);\n}\n";
    else if (kind == MSCAN)
        o << "extern \"C\" __global__ __launch_bounds__(256) void " << entry_name(kind, C, D, sh) << "(const vdl::MsArgs Cr, const vdl::MScanDesc *__restrict__ Dp) {\n"
             "    constexpr vdl::MsArgs C = vdl::jit_args();\n"
             "    constexpr vdl::MScanDesc D = vdl::jit_desc();\n"
             "    vdl::mscan_body<" << sh.nc << ", " << sh.u << ", " << b << ", " << b << ", " << (sh.grouped ? "true" : "false") << ", " << (sh.der ? "true" : "false")
          << ", " << (C.lazy ? "true" : "false") << ">(C, Cr, D, *Dp);\n}\n";
    else if (kind == SELECT)
        o << "extern \"C\" __global__ __launch_bounds__(256) void " << entry_name(kind) << "(const vdl::MsArgs Cr, const vdl::MScanDesc *__restrict__ Dp) {\n"
             "    constexpr vdl::MsArgs C = vdl::jit_args();\n"
             "    constexpr vdl::MScanDesc D = vdl::jit_desc();\n"
             "    vdl::project_select_body<" << sh.nc << ", vdl::kProjU, " << b << ", " << b << ">(C, Cr, D, *Dp);\n}\n";
    else
        o << "extern \"C\" __global__ __launch_bounds__(256) void " << entry_name(kind) << "(const vdl::MsArgs Cr, const vdl::MScanDesc *__restrict__ Dp, const uint16_t *__restrict__ scratch,\n"
             "        const int64_t *__restrict__ counts, const int64_t *__restrict__ offsets) {\n"
             "    constexpr vdl::MsArgs C = vdl::jit_args();\n"
             "    constexpr vdl::MScanDesc D = vdl::jit_desc();\n"
             "    vdl::project_take_body<" << sh.nc << ">(C, Cr, D, *Dp, scratch, counts, offsets);\n}\n";
    return o.str();
}
std::string mscan_source(const MsArgs &C, const MScanDesc &D, const Shape &sh) { return scan_source(MSCAN, C, D, sh); }
// the fused front in one pass: two descriptors -- the deciding columns as the select side numbers them, every column with the outputs
std::string front_source(const MsArgs &Cs, const MScanDesc &Ds, const MsArgs &Ct, const MScanDesc &Dt, const Shape &sh, int nct) {
    std::ostringstream o;
    o << "#define VDL_SPEC_UNROLL _Pragma(\"unroll\")\n";
    if (sh.rt_bounds) o << "#define VDL_RT_BOUNDS 1\n";
    if (has_sat_diff(Cs, Ds) || has_sat_diff(Ct, Dt)) o << "#define VDL_SAT_DIFF 1\n";
    if (has_lookup_decode(Cs) || has_lookup_decode(Ct)) o << "#define VDL_LOOKUP_DECODE 1\n";
    o << "#define VDL_PROJ_U " << VDL_PROJ_U_HOST << "\n#define VDL_FRONT_BATCH " << VDL_FRONT_BATCH_HOST << "\n" << kEmbedded << "\n" << desc_text(SELECT, Cs, Ds, "_s", sh.rt_bounds) << desc_text(TAKE, Ct, Dt, "_t", sh.rt_bounds);
    const char *b = sh.vec ? "true" : "false";
    // (Q3's front: 107 VGPRs = 4 blocks per CU; asked to fit 5 or 6 waves per SIMD -- 96 / 80 registers, 12 / 76 bytes of scratch -- the pass
    // took the same 2.64-2.66 ms at SF100: it moves 14.7 GB, i.e. 5.5 TB/s, and is bound by that, not by occupancy)
    o << "extern \"C\" __global__ __launch_bounds__(256) void " << entry_name(FRONT) << "(const vdl::MsArgs Csr, const vdl::MScanDesc *__restrict__ Dsp, const vdl::MsArgs Ctr,\n"
         "        const vdl::MScanDesc *__restrict__ Dtp, const vdl::FrontLook lk) {\n"
         "    constexpr vdl::MsArgs Cs = vdl::jit_args_s();\n"
         "    constexpr vdl::MScanDesc Ds = vdl::jit_desc_s();\n"
         "    constexpr vdl::MsArgs Ct = vdl::jit_args_t();\n"
         "    constexpr vdl::MScanDesc Dt = vdl::jit_desc_t();\n"
         "    vdl::project_front_body<" << sh.nc << ", " << nct << ", vdl::kProjU, " << b << ", " << b << ">(Cs, Csr, Ds, *Dsp, Ct, Ctr, Dt, *Dtp, lk);\n}\n";
    return o.str();
}
const char *entry_name(Kind kind) { return kind == MSCAN ? "vdl_jit_mscan" : kind == SELECT ? "vdl_jit_project_select" : kind == FRONT ? "vdl_jit_project_front" : "vdl_jit_project_take"; }
// aggregate scans carry their shape in the kernel's name, so that a profile of a tuned run lists the tuner's candidates apart
std::string entry_name(Kind kind, const MsArgs &C, const MScanDesc &D, const Shape &sh) {
    if (kind != MSCAN) return entry_name(kind);
    char tag[16];
    snprintf(tag, sizeof tag, "%06llx", (unsigned long long)(fnv(desc_text(kind, C, D, "", sh.rt_bounds)) & 0xffffffull));      // which plan's scan (run-time bounds: which shape of plan)
    // (staged: how many filter columns come with the tile is part of the name too -- the profiles tell the forms apart by it)
    int eager_filters = 0;
    for (int c = 0; c < C.ncol; c++) eager_filters += ((C.filtered >> c) & 1u) && !((C.derived >> c) & 1u) && C.stage(c) == 0;
    return std::string("vdl_jit_mscan_") + (sh.grouped ? "grouped_" : "") + (C.packed ? "packed_" : "") + "u" + std::to_string(sh.u) + (C.lazy ? "_staged" + std::to_string(eager_filters) + "_" : "_") +
           (sh.census ? "census_" : "") + tag + (sh.batch ? "_batch" + std::to_string(sh.batch) : "") + (sh.rt_bounds ? "_rtb" : "") + (sh.wide ? "_wide" : "");
}

bool compile(const std::string &src, const std::string &arch, std::vector<char> &code, std::string &log, Origin *origin) {
    if (origin) *origin = COMPILED;
    std::string key = std::to_string(fnv(src)) + "_" + std::to_string(src.size()) + "_" + arch;
    {
        Rtc &r0 = rtc();
        int major = 0, minor = 0;
        if (r0.lib && r0.version && r0.version(&major, &minor) == 0) key += "_rtc" + std::to_string(major) + "." + std::to_string(minor);
    }
    {
        std::lock_guard<std::mutex> g(g_mu);
        auto it = g_code.find(key);
        if (it != g_code.end()) { code = it->second; g_from_memory++; if (origin) *origin = FROM_MEMORY; return true; }
    }
    if (const char *dump = getenv("VDL_JIT_DUMP")) {           // debugging: the generated translation unit as a file
        std::ofstream f(std::string(dump) + "/vdl_" + key + ".hip");
        f << src;
    }
    const std::string dir = trusted_cache_dir();
    std::string path;
    if (!dir.empty()) {
        path = dir + "/vdl_" + key + ".vdlco";
        if (cache_read(path, src, code)) { std::lock_guard<std::mutex> g(g_mu); g_code[key] = code; g_from_disk++; if (origin) *origin = FROM_DISK; return true; }
    }
    Rtc &r = rtc();
    if (!r.lib || !r.why.empty()) { log = r.why.empty() ? "libhiprtc not usable" : r.why; return false; }
    void *prog = nullptr;
    if (r.create(&prog, src.c_str(), "vdl_jit_scan.hip", 0, nullptr, nullptr) != 0) { log = "hiprtcCreateProgram failed"; return false; }
    const std::string a = "--offload-arch=" + arch;
    const char *opts[] = {a.c_str(), "-O3", "-std=c++17"};
    const int rc = r.compile(prog, 3, opts);
    size_t n = 0;
    if (r.log_size(prog, &n) == 0 && n > 1) { log.resize(n); r.log(prog, &log[0]); }
    if (rc != 0) { if (log.empty()) log = "hiprtcCompileProgram failed (" + std::to_string(rc) + ")"; r.destroy(&prog); return false; }
    n = 0;
    r.code_size(prog, &n);
    code.resize(n);
    r.code(prog, code.data());
    r.destroy(&prog);
    if (code.empty()) { log = "hiprtc produced no code"; return false; }
    if (!path.empty()) cache_write(path, src, code);
    g_compiled++;
    std::lock_guard<std::mutex> g(g_mu);
    g_code[key] = code;
    return true;
}

Kernel::~Kernel() { if (mod) (void)hipModuleUnload(mod); }

std::shared_ptr<Kernel> load(const std::vector<char> &code, std::string &why, const std::string &entry) {
    auto k = std::make_shared<Kernel>();
    hipError_t e = hipModuleLoadData(&k->mod, code.data());
    if (e != hipSuccess) { why = std::string("hipModuleLoadData: ") + hipGetErrorString(e); k->mod = nullptr; return nullptr; }
    e = hipModuleGetFunction(&k->fn, k->mod, entry.c_str());
    if (e != hipSuccess) { why = std::string("hipModuleGetFunction: ") + hipGetErrorString(e); return nullptr; }
    return k;
}

}  // namespace jit
}  // namespace vdl
