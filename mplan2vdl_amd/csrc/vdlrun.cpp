// vdlrun -- the executor end of the reference's pipe:
//   ./tpchrun DIR plan.mplan | sed 's/;;.*//' | vdlrun --rows N            (synthetic TPC-H-shaped lineitem)
//   ./tpchrun DIR plan.mplan | sed 's/;;.*//' | vdlrun --data COLDIR       (exported columns, see below)
// reads VDL text on stdin, runs it on the GPU through libvdl and prints the JSON document that
// /root/reference/resolve.py:8-32 consumes: {"results": {"tmpN": {".name": [...]}}, "timings": {...}}.
// Exit status is non-zero on any error (resolve.py:42-43 treats a missing "results" key as failure).
// --data COLDIR: COLDIR/columns.csv lists "<table.col>,<bytes per element>,<rows>" and COLDIR/<table.col>.bin holds
// the raw little-endian array (what mplan2vdl_amd.catalog.export_columns writes; a MonetDB BAT tail file of a
// fixed-width column has the same layout).  Only the columns the program Loads are read.
//   ... | vdlrun --gpus N [--shard TABLE] --rows M | --data COLDIR        one process per GPU (SURVEY.md section 8(b),(e))
// --gpus N forks N ranks BEFORE anything touches HIP; rank r opens device r, holds rows [r*n/N, (r+1)*n/N) of the sharded
// table (--shard, default lineitem) and the other tables in full, joins an RCCL communicator (rank 0's id travels through a
// file in a private temporary directory) and calls vdl_run_sharded.  The parent prints ONE reply: the common answer of a
// fold plan, or the ranks' slices concatenated in rank order for a plan with a Partition.
//   ... | vdlrun --encode ...                                                  columns read through their images
// --encode builds the frame-of-reference image of every column it uploads or generates (vdl_encode_column; each rank of its own
// rows), so that the scans read the narrow copies; after the run one line "vdlrun: images: <vdl_plan_image_columns>" goes to
// stderr (rank 0's).  The reply on stdout is the same as without it.
//   ... | vdlrun --encode-steps ...                                             join indices read through their step images
// --encode-steps tries a step image (vdl_encode_steps) on every column it uploads or generates: a column that never decreases and
// steps by at most 1 -- a clustered join index -- gets one, and fronts, dimension and semi-join scans read it.  After the run one
// line "vdlrun: step images: <vdl_plan_step_columns>" goes to stderr beside the images line; it is also printed when --encode runs
// under VDL_STEP_IMAGES=1, which makes vdl_encode_column try a step image too.
//   ... | vdlrun --encode --lookup-images ...                                   join lookups read the dimension columns' images
// --lookup-images switches vdl_set_lookup_images on: a dimension column looked up through a join index is read from its image
// (built by --encode) where its use allows.  After the run one line "vdlrun: lookup images: <vdl_plan_lookup_columns>" goes to
// stderr (rank 0's); it is also printed under VDL_LOOKUP_IMAGES=1, which switches them on when the context opens.
//   ... | vdlrun --order-by revenue:desc,o_orderdate__orders__o_orderdate --limit 10 ...      ORDER BY / LIMIT on the device
// --order-by FIELD[:asc|:desc][:text[=HEAP]],... names outputs by their full field name or their tmpN key, --limit N keeps the first N
// rows (vdl_plan_set_order); :text orders the key by its strings (vdl_plan_set_order_text) over HEAP, or over table.col.heap for a
// field named col__table__col, and --data uploads that heap too.  The reply has the same shape with shorter, ordered lists, so
// resolve.py decodes it untouched.  With --gpus only together with --order-sharded (vdl_plan_set_order_sharded): the ranks then run, every
// rank ends with the whole ordered answer -- on the exchange route the ranks' first rows are merged on the device, --limit 1 .. 4096 --,
// the rank replies are marked replicated and ONE of them is printed.  Without it --gpus refuses an order before any rank starts.
//   ... | vdlrun --jit --batch b.vdl --batch c.vdl ...                             several programs, one pass where they can share it
// --batch FILE (repeatable; needs --jit or --jit-tune): the program on stdin and the programs in the files run as ONE vdl_run_batch --
// those that differ in their literals alone share one scan of the columns, the others run alone inside the same call -- and one reply
// is printed per line, stdin's first.  The options (--order-by included) apply to every program.  One line per program "vdlrun:
// batch: <vdl_plan_batch_note>" goes to stderr.  With --gpus only together with --batch-sharded.
//   ... | vdlrun --gpus N --jit --batch b.vdl --batch-sharded ...                  several programs in one sharded call
// --batch-sharded (needs --gpus, --batch and --jit or --jit-tune): every rank calls vdl_run_batch_sharded with the programs -- those that
// fuse as a whole on the fold route share ONE all-gather and ONE merge, the others run through vdl_run_sharded inside the call -- the rank
// replies are marked replicated and rank 0's are printed, stdin's first, then the --batch programs' in their order.  One line per program
// "vdlrun: batch-sharded: <vdl_plan_batch_sharded_note>; <vdl_plan_batch_note>" goes to stderr (rank 0's).  Without it --gpus refuses
// --batch before any rank starts: vdl_run_sharded takes one plan.
//   ... | vdlrun --wide-sums ...  |  vdlrun --checked-sums ...                       exact 128-bit SUM results
// --wide-sums (vdl_plan_set_wide_sums 1): the reply keeps its shape and every value is printed as the exact decimal integer, of any
// size (JSON has no limit; Python's json reads them as ints and resolve.py passes ints through).  --checked-sums (mode 2): a value
// outside int64 fails the run, the message naming output, group and value, and vdlrun exits non-zero.  Fused plans only.
// VDL_WIDE_SUMS=1|2 in the environment does the same when no option is given.  With --gpus only together with --wide-sharded
// (vdl_plan_set_wide_sums_sharded; VDL_WIDE_SHARDED=1 does the same): the ranks merge their (lo, hi) partial words with carry, every rank
// ends with the exact answer of the whole table and ONE reply is printed, in exact decimals; --checked-sums is then checked on the merged
// values.  Without it --gpus refuses the switch before any rank starts, as every sharded entry point does.
// --wide-tail (vdl_plan_set_wide_sums_tail; only together with --wide-sums | --checked-sums, on one GPU): plans that do not fuse as a
// whole run too -- their sums through the per-operator folds, exact where delivered and checked where another statement reads them.
// --batch-grouped: programs whose one scan is a GROUP BY over table columns share a grouped batch too (vdl_set_batch_grouped); without it
// they run alone, as "grouped scans are not batched".
// --batch-joins: programs whose one scan has derived columns or a prelude (join scans) share a batch too (vdl_set_batch_joins); without
// it they run alone, as "scans with derived columns are not batched" / "scans with lookup tables or semi-join sets are not batched".
#include <signal.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <cstring>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "vdl.h"

namespace {
struct GenSpec { const char *name; int width; int64_t lo, hi, mul, add; };
// value ranges: /root/reference/tests/tpch10noorder/bounds.csv:59-79
const GenSpec kLineitem[] = {
    {"lineitem.l_shipdate", 4, 727564, 730089, 1, 0},      {"lineitem.l_discount", 8, 0, 10, 1, 0},
    {"lineitem.l_quantity", 8, 1, 50, 100, 0},             {"lineitem.l_extendedprice", 8, 90091, 10494950, 1, 0},
    {"lineitem.l_tax", 8, 0, 8, 1, 0},                     {"lineitem.l_returnflag", 4, 0, 2, 24, 16},
    {"lineitem.l_linestatus", 4, 0, 1, 24, 16},
};

struct ColFile { int width; int64_t rows; };

int load_data_dir(vdl_ctx *ctx, const std::string &dir, const std::string &program, const std::string &shard_table = "", int rank = 0, int world = 1,
                  int64_t *row0_out = nullptr, bool encode = false, bool encode_steps = false) {
    std::map<std::string, ColFile> listed;
    std::ifstream manifest(dir + "/columns.csv");
    if (!manifest) { std::fprintf(stderr, "vdlrun: cannot read %s/columns.csv\n", dir.c_str()); return 1; }
    std::string line;
    while (std::getline(manifest, line)) {
        std::istringstream ls(line);
        std::string name, w, r;
        if (!std::getline(ls, name, ',') || !std::getline(ls, w, ',') || !std::getline(ls, r, ',')) continue;
        listed[name] = ColFile{std::atoi(w.c_str()), std::atoll(r.c_str())};
    }
    std::istringstream prog(program);
    while (std::getline(prog, line)) {
        const size_t at = line.find(",Load,");
        if (at == std::string::npos) continue;
        std::string name = line.substr(at + 6);
        const size_t cut = name.find(";;");
        if (cut != std::string::npos) name.resize(cut);
        while (!name.empty() && isspace((unsigned char)name.back())) name.pop_back();
        auto it = listed.find(name);
        if (it == listed.end()) { std::fprintf(stderr, "vdlrun: column %s is not in %s/columns.csv\n", name.c_str(), dir.c_str()); return 1; }
        if (it->second.rows < 0) continue;                 // uploaded already
        // a column of the sharded table: this rank's row range only (string heaps "table.col.heap" are not row-aligned: whole)
        int64_t lo = 0, hi = it->second.rows;
        const bool is_heap = name.size() > 5 && name.compare(name.size() - 5, 5, ".heap") == 0;
        if (world > 1 && !shard_table.empty() && !is_heap && name.compare(0, shard_table.size() + 1, shard_table + ".") == 0) {
            lo = it->second.rows * rank / world; hi = it->second.rows * (rank + 1) / world;
            if (row0_out) *row0_out = lo;
        }
        const size_t bytes = (size_t)it->second.width * (size_t)(hi - lo);
        std::vector<char> buf(bytes ? bytes : 1);
        std::ifstream f(dir + "/" + name + ".bin", std::ios::binary);
        if (f) f.seekg((std::streamoff)((size_t)it->second.width * (size_t)lo));
        if (!f || (bytes && !f.read(buf.data(), (std::streamsize)bytes))) {
            std::fprintf(stderr, "vdlrun: %s/%s.bin is missing or shorter than the %lld rows columns.csv lists\n", dir.c_str(), name.c_str(), (long long)it->second.rows);
            return 1;
        }
        int rc = vdl_upload_column(ctx, name.c_str(), buf.data(), it->second.width, hi - lo);
        if (rc) { std::fprintf(stderr, "vdlrun: vdl_upload_column(%s) failed (%d): %s\n", name.c_str(), rc, vdl_last_error(ctx)); return 1; }
        if (encode && (rc = vdl_encode_column(ctx, name.c_str()))) {
            std::fprintf(stderr, "vdlrun: vdl_encode_column(%s) failed (%d): %s\n", name.c_str(), rc, vdl_last_error(ctx));
            return 1;
        }
        if (encode_steps && (rc = vdl_encode_steps(ctx, name.c_str()))) {
            std::fprintf(stderr, "vdlrun: vdl_encode_steps(%s) failed (%d): %s\n", name.c_str(), rc, vdl_last_error(ctx));
            return 1;
        }
        listed.erase(it);                                  // a column loaded twice by the program is uploaded once
        listed[name] = ColFile{0, -1};
    }
    return 0;
}

int die(vdl_ctx *c, const char *what, int rc) {
    std::fprintf(stderr, "vdlrun: %s failed (%d): %s\n", what, rc, c ? vdl_last_error(c) : "");
    return 1;
}
struct Reply {
    struct Out { std::string name, tmp; std::vector<int64_t> vals; std::vector<int64_t> hi; };      // hi: --wide-sums / --checked-sums, bits 64..127 of every value
    std::vector<Out> outs;
    std::vector<std::pair<std::string, double>> timings;
    bool replicated = true;          // every rank holds the whole answer (fold plans) / this is one rank's slice (Partition plans)
};

void collect(vdl_plan *plan, Reply &r) {
    for (int k = 0; k < vdl_n_outputs(plan); k++) {
        const char *name, *tmp; const int64_t *vals; size_t n;
        vdl_output(plan, k, &name, &tmp, &vals, &n);
        r.outs.push_back({name, tmp, std::vector<int64_t>(vals, vals + n), {}});
        const int64_t *hi = nullptr;
        if (vdl_output_high(plan, k, &hi, nullptr) == VDL_OK && hi) r.outs.back().hi.assign(hi, hi + n);
    }
    for (int k = 0; k < vdl_n_timings(plan); k++) {
        const char *label; double us;
        vdl_timing(plan, k, &label, &us);
        r.timings.push_back({label, us});
    }
}

// (hi << 64) | lo as a decimal integer of any size: JSON has no upper limit for one
std::string wide_decimal(int64_t lo, int64_t hi) {
    unsigned __int128 u = ((unsigned __int128)(uint64_t)hi << 64) | (uint64_t)lo;
    if (hi < 0) u = (unsigned __int128)0 - u;
    std::string s;
    do { s.insert(s.begin(), (char)('0' + (int)(u % 10))); u /= 10; } while (u != 0);
    return hi < 0 ? "-" + s : s;
}

void print_reply(const Reply &r) {
    std::printf("{\"results\": {");
    for (size_t k = 0; k < r.outs.size(); k++) {
        std::printf("%s\"%s\": {\".%s\": [", k ? ", " : "", r.outs[k].tmp.c_str(), r.outs[k].name.c_str());
        for (size_t i = 0; i < r.outs[k].vals.size(); i++) {
            if (i < r.outs[k].hi.size()) std::printf("%s%s", i ? ", " : "", wide_decimal(r.outs[k].vals[i], r.outs[k].hi[i]).c_str());      // wide sums: the exact value
            else std::printf("%s%lld", i ? ", " : "", (long long)r.outs[k].vals[i]);
        }
        std::printf("]}");
    }
    std::printf("}, \"timings\": {");
    for (size_t k = 0; k < r.timings.size(); k++) std::printf("%s\"%s\": %.0f", k ? ", " : "", r.timings[k].first.c_str(), r.timings[k].second);
    std::printf("}}\n");
}

bool write_reply(const std::string &path, const Reply &r) {
    std::ofstream f(path + ".tmp", std::ios::binary);
    f << (r.replicated ? 1 : 0) << "\n" << r.outs.size() << "\n";
    for (const auto &o : r.outs) {
        f << o.name << "\n" << o.tmp << "\n" << o.vals.size() << "\n";
        f.write((const char *)o.vals.data(), (std::streamsize)(sizeof(int64_t) * o.vals.size()));
        f << "\n" << o.hi.size() << "\n";                      // (wide sums: the high words travel with their values)
        f.write((const char *)o.hi.data(), (std::streamsize)(sizeof(int64_t) * o.hi.size()));
        f << "\n";
    }
    f << r.timings.size() << "\n";
    for (const auto &t : r.timings) f << t.first << "\n" << t.second << "\n";
    f.close();
    return f.good() && std::rename((path + ".tmp").c_str(), path.c_str()) == 0;
}

bool read_reply(const std::string &path, Reply &r) {
    std::ifstream f(path, std::ios::binary);
    std::string line;
    auto num = [&]() { std::getline(f, line); return std::atoll(line.c_str()); };
    if (!f) return false;
    r.replicated = num() != 0;
    const long long nouts = num();
    for (long long k = 0; k < nouts; k++) {
        Reply::Out o;
        std::getline(f, o.name); std::getline(f, o.tmp);
        o.vals.resize((size_t)num());
        f.read((char *)o.vals.data(), (std::streamsize)(sizeof(int64_t) * o.vals.size()));
        std::getline(f, line);
        o.hi.resize((size_t)num());
        f.read((char *)o.hi.data(), (std::streamsize)(sizeof(int64_t) * o.hi.size()));
        std::getline(f, line);
        r.outs.push_back(std::move(o));
    }
    const long long nt = num();
    for (long long k = 0; k < nt; k++) { std::string label; std::getline(f, label); std::getline(f, line); r.timings.push_back({label, std::atof(line.c_str())}); }
    return (bool)f || f.eof();
}

struct Options {
    int64_t rows = 60175;           // SF0.01 lineitem, /root/reference/tests/tpchnoorder/bounds.csv:59
    uint64_t seed = 0x5EED0006ULL;
    int device = 0, fuse = 1, profile = 0, describe = 0, gpus = 1, jit = 0, jit_share = 0, encode = 0, encode_steps = 0, order_sharded = 0, batch_grouped = 0, batch_joins = 0, batch_sharded = 0, lookup_images = 0;
    int wide = -1;                  // --wide-sums 1 / --checked-sums 2; -1: as the plan was parsed (VDL_WIDE_SUMS)
    int wide_sharded = 0;           // --wide-sharded: vdl_plan_set_wide_sums_sharded
    int wide_tail = 0;              // --wide-tail: vdl_plan_set_wide_sums_tail (only together with --wide-sums | --checked-sums)
    std::string data_dir, shard = "lineitem";
    std::vector<std::string> order_fields;
    std::vector<int> order_desc;
    std::vector<std::string> order_heaps;       // per key: the heap of a :text key, "" otherwise
    long long limit = 0;
    std::vector<std::string> batch_files;       // --batch
    std::vector<std::string> batch_texts;       // ... and what they hold
};

// "a:desc,b,c:asc:text,d:text=t.c.heap" -> fields, directions and text heaps ("" = no text key); false = malformed (empty list or
// field, unknown or repeated modifier, a text key whose heap is neither given nor derivable from the field's name)
bool parse_order_by(const std::string &list, Options &o) {
    size_t at = 0;
    if (list.empty()) return false;
    for (;;) {
        const size_t comma = list.find(',', at);
        std::string item = list.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
        int desc = 0;
        bool have_dir = false, text = false;
        std::string heap;
        size_t colon = item.find(':');
        const std::string field = item.substr(0, colon);
        while (colon != std::string::npos) {
            const size_t next = item.find(':', colon + 1);
            const std::string mod = item.substr(colon + 1, next == std::string::npos ? std::string::npos : next - colon - 1);
            if ((mod == "asc" || mod == "desc") && !have_dir) { have_dir = true; desc = mod == "desc"; }
            else if (mod == "text" && !text) text = true;
            else if (mod.compare(0, 5, "text=") == 0 && mod.size() > 5 && !text) { text = true; heap = mod.substr(5); }
            else return false;
            colon = next;
        }
        if (field.empty()) return false;
        if (text && heap.empty()) {
            // col__table__col (how the compiler names a column's output) -> table.col.heap
            const size_t a1 = field.find("__"), a2 = a1 == std::string::npos ? a1 : field.find("__", a1 + 2);
            if (a2 == std::string::npos || a1 == 0 || a2 == a1 + 2 || a2 + 2 >= field.size() || field.find("__", a2 + 2) != std::string::npos) {
                std::fprintf(stderr, "vdlrun: --order-by %s:text: no heap can be derived from this field (only from col__table__col, as table.col.heap); "
                                     "name it with :text=HEAP\n", field.c_str());
                return false;
            }
            heap = field.substr(a1 + 2, a2 - a1 - 2) + "." + field.substr(a2 + 2) + ".heap";
        }
        o.order_fields.push_back(field);
        o.order_desc.push_back(desc);
        o.order_heaps.push_back(heap);
        if (comma == std::string::npos) return true;
        at = comma + 1;
    }
}

// one rank of `world` (world = 1 without --gpus: plain vdl_run); comm_dir = where rank 0 leaves the communicator id
// (more: the replies of the --batch programs, in their order)
int run_rank(const Options &o, const std::string &text, int rank, int world, const std::string &comm_dir, Reply &reply, std::vector<Reply> *more = nullptr) {
    vdl_ctx *ctx = nullptr;
    int rc = vdl_open(&ctx, o.describe ? -1 : (world > 1 || !comm_dir.empty() ? rank : o.device));
    if (rc) return die(ctx, "vdl_open", rc);
    if (o.batch_grouped) vdl_set_batch_grouped(ctx, 1);
    if (o.batch_joins) vdl_set_batch_joins(ctx, 1);
    if (o.lookup_images) vdl_set_lookup_images(ctx, 1);
    std::vector<vdl_plan *> plans;
    std::string loads = text;                                  // every program's text: what --data looks for Loads in
    for (size_t k = 0; k <= o.batch_texts.size(); k++) {
        const std::string &t = k ? o.batch_texts[k - 1] : text;
        if (k) loads += "\n" + t;
        vdl_plan *one = nullptr;
        if ((rc = vdl_parse(ctx, t.data(), t.size(), &one))) return die(ctx, "vdl_parse", rc);
        vdl_plan_set_fusion(one, o.fuse);
        vdl_plan_set_profiling(one, o.profile);
        if (o.jit) vdl_plan_set_jit(one, o.jit);
        if (o.jit_share) vdl_plan_set_jit_bounds(one, 1);
        if (o.wide >= 0 && (rc = vdl_plan_set_wide_sums(one, o.wide))) return die(ctx, "vdl_plan_set_wide_sums", rc);
        if (o.wide_sharded && (rc = vdl_plan_set_wide_sums_sharded(one, 1))) return die(ctx, "vdl_plan_set_wide_sums_sharded", rc);
        if (o.wide_tail && (rc = vdl_plan_set_wide_sums_tail(one, 1))) return die(ctx, "vdl_plan_set_wide_sums_tail", rc);
        if (!o.order_fields.empty() || o.limit > 0) {
            std::vector<const char *> fields;
            for (const std::string &f : o.order_fields) fields.push_back(f.c_str());
            if ((rc = vdl_plan_set_order(one, (int)fields.size(), fields.data(), o.order_desc.data(), o.limit))) return die(ctx, "vdl_plan_set_order", rc);
            for (size_t q = 0; q < o.order_heaps.size(); q++)
                if (!o.order_heaps[q].empty() && (rc = vdl_plan_set_order_text(one, o.order_fields[q].c_str(), o.order_heaps[q].c_str()))) return die(ctx, "vdl_plan_set_order_text", rc);
            if (o.order_sharded) vdl_plan_set_order_sharded(one, 1);
        }
        plans.push_back(one);
        if (o.describe) break;
    }
    vdl_plan *plan = plans[0];
    if (o.describe) { std::fputs(vdl_plan_describe(plan), stdout); return 0; }
    int64_t row0 = 0;
    if (!o.data_dir.empty()) {
        // the heaps of text keys are read by the order step, whether or not a program Loads them
        for (const std::string &h : o.order_heaps) if (!h.empty()) loads += "\n0,Load," + h;
        if (load_data_dir(ctx, o.data_dir, loads, o.shard, rank, world, &row0, o.encode != 0, o.encode_steps != 0)) return 1;
    } else {
        row0 = o.rows * rank / world;
        const int64_t mine = o.rows * (rank + 1) / world - row0;
        for (const GenSpec &g : kLineitem)
            if ((rc = vdl_generate_column(ctx, g.name, g.width, row0, mine, o.seed, g.lo, g.hi, g.mul, g.add))) return die(ctx, "vdl_generate_column", rc);
        if (o.encode)
            for (const GenSpec &g : kLineitem) if ((rc = vdl_encode_column(ctx, g.name))) return die(ctx, "vdl_encode_column", rc);
        if (o.encode_steps)
            for (const GenSpec &g : kLineitem) if ((rc = vdl_encode_steps(ctx, g.name))) return die(ctx, "vdl_encode_steps", rc);
    }
    if (comm_dir.empty() && plans.size() > 1) {
        if ((rc = vdl_run_batch(ctx, plans.data(), (int)plans.size()))) return die(ctx, "vdl_run_batch", rc);
        for (vdl_plan *one : plans) std::fprintf(stderr, "vdlrun: batch: %s\n", vdl_plan_batch_note(one));
    } else if (comm_dir.empty()) {
        if ((rc = vdl_run(ctx, plan))) return die(ctx, "vdl_run", rc);
    } else {
        unsigned char id[VDL_COMM_ID_BYTES];
        const std::string id_path = comm_dir + "/id";
        if (rank == 0) {
            if ((rc = vdl_comm_unique_id(id))) return die(ctx, "vdl_comm_unique_id", rc);
            std::ofstream f(id_path + ".tmp", std::ios::binary);
            f.write((const char *)id, sizeof id);
            f.close();
            if (!f.good() || std::rename((id_path + ".tmp").c_str(), id_path.c_str())) { std::fprintf(stderr, "vdlrun: cannot write %s\n", id_path.c_str()); return 1; }
        } else {
            bool got = false;
            for (int tries = 0; tries < 6000 && !got; tries++) {          // up to 60 s for rank 0 to get there
                std::ifstream f(id_path, std::ios::binary);
                got = f && f.read((char *)id, sizeof id);
                if (!got) usleep(10000);
            }
            if (!got) { std::fprintf(stderr, "vdlrun: rank %d never saw the communicator id\n", rank); return 1; }
        }
        if ((rc = vdl_comm_init(ctx, rank, world, id))) return die(ctx, "vdl_comm_init", rc);
        for (vdl_plan *one : plans) { vdl_plan_set_sharded_table(one, o.shard.c_str()); vdl_plan_set_row_offset(one, row0); }
        if (o.batch_sharded) {
            // every program in ONE sharded call; what the call leaves on a rank is taken as the answer (rank 0's is printed)
            reply.replicated = true;
            if ((rc = vdl_run_batch_sharded(ctx, plans.data(), (int)plans.size()))) return die(ctx, "vdl_run_batch_sharded", rc);
            if (rank == 0)
                for (vdl_plan *one : plans) std::fprintf(stderr, "vdlrun: batch-sharded: %s; %s\n", vdl_plan_batch_sharded_note(one), vdl_plan_batch_note(one));
        } else {
            int whole = 0;
            const char *route = nullptr;
            if ((rc = vdl_plan_sharded_route(ctx, plan, &route, &whole))) return die(ctx, "vdl_plan_sharded_route", rc);
            reply.replicated = whole != 0;
            if ((rc = vdl_run_sharded(ctx, plan))) return die(ctx, "vdl_run_sharded", rc);
        }
    }
    collect(plan, reply);
    for (size_t k = 1; k < plans.size() && more; k++) { more->emplace_back(); collect(plans[k], more->back()); }
    if (o.encode && rank == 0) {
        const char *list = "";
        vdl_plan_image_columns(plan, &list);
        std::fprintf(stderr, "vdlrun: images: %s\n", list);
    }
    const char *by_env = std::getenv("VDL_STEP_IMAGES");
    if ((o.encode_steps || (o.encode && by_env && *by_env && *by_env != '0')) && rank == 0) {
        const char *list = "";
        vdl_plan_step_columns(plan, &list);
        std::fprintf(stderr, "vdlrun: step images: %s\n", list);
    }
    const char *lk_env = std::getenv("VDL_LOOKUP_IMAGES");
    if ((o.lookup_images || (lk_env && *lk_env && *lk_env != '0')) && rank == 0) {
        const char *list = "";
        vdl_plan_lookup_columns(plan, &list);
        std::fprintf(stderr, "vdlrun: lookup images: %s\n", list);
    }
    for (vdl_plan *one : plans) vdl_plan_free(one);
    vdl_close(ctx);
    return 0;
}
}  // namespace

int main(int argc, char **argv) {
    Options o;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        if (a == "--rows" && i + 1 < argc) o.rows = std::atoll(argv[++i]);
        else if (a == "--data" && i + 1 < argc) o.data_dir = argv[++i];
        else if (a == "--seed" && i + 1 < argc) o.seed = std::strtoull(argv[++i], nullptr, 0);
        else if (a == "--device" && i + 1 < argc) o.device = std::atoi(argv[++i]);
        else if (a == "--gpus" && i + 1 < argc) o.gpus = std::atoi(argv[++i]);
        else if (a == "--shard" && i + 1 < argc) o.shard = argv[++i];
        else if (a == "--batch" && i + 1 < argc) o.batch_files.push_back(argv[++i]);
        else if (a == "--batch-grouped") o.batch_grouped = 1;
        else if (a == "--batch-joins") o.batch_joins = 1;
        else if (a == "--batch-sharded") o.batch_sharded = 1;
        else if (a == "--lookup-images") o.lookup_images = 1;
        else if (a == "--wide-sums") o.wide = 1;
        else if (a == "--checked-sums") o.wide = 2;
        else if (a == "--wide-sharded") o.wide_sharded = 1;
        else if (a == "--wide-tail") o.wide_tail = 1;
        else if (a == "--order-by" && i + 1 < argc && parse_order_by(argv[i + 1], o)) i++;
        else if (a == "--order-sharded") o.order_sharded = 1;
        else if (a == "--limit" && i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9' && std::strspn(argv[i + 1], "0123456789") == std::strlen(argv[i + 1]) &&
                 std::strlen(argv[i + 1]) <= 18) o.limit = std::atoll(argv[++i]);
        else if (a == "--no-fuse") o.fuse = 0;
        else if (a == "--jit") o.jit = 1;
        else if (a == "--encode") o.encode = 1;
        else if (a == "--encode-steps") o.encode_steps = 1;
        else if (a == "--jit-tune") o.jit = 2;
        else if (a == "--jit-share") o.jit_share = 1;      // filter bounds at run time: queries that differ in literals alone share the specialised code
        else if (a == "--profile") o.profile = 1;
        else if (a == "--describe") o.describe = 1;
        else {
            std::fprintf(stderr, "usage: vdlrun [--rows N | --data DIR] [--gpus N [--shard TABLE]] [--order-by FIELD[:asc|:desc][:text[=HEAP]],... ] [--limit N] [--order-sharded] [--batch FILE ...] [--batch-grouped] [--batch-joins] [--batch-sharded] [--seed S] [--device D] [--no-fuse] [--jit | --jit-tune] [--jit-share] [--encode] [--encode-steps] [--lookup-images] [--wide-sums | --checked-sums] [--wide-sharded] [--profile] [--describe] < program.vdl\n");
            return 2;
        }
    }
    if (!o.batch_files.empty() && !o.jit) {                    // (only specialised scans are batched: without --jit every program would run alone)
        std::fprintf(stderr, "usage: vdlrun --batch FILE needs --jit or --jit-tune: a batch shares a scan specialised for its plans\n");
        return 2;
    }
    if (o.wide_tail && o.wide <= 0) {                          // (the tail switch says how a WIDE plan runs)
        std::fprintf(stderr, "usage: vdlrun --wide-tail needs --wide-sums or --checked-sums: it lets a plan with wide sums on run through the per-operator folds\n");
        return 2;
    }
    if (o.gpus < 1 || o.gpus > 128) { std::fprintf(stderr, "vdlrun: --gpus must be 1 .. 128\n"); return 2; }
    std::string text((std::istreambuf_iterator<char>(std::cin)), std::istreambuf_iterator<char>());
    bool sharded = false;
    for (int i = 1; i < argc; i++) sharded = sharded || std::string(argv[i]) == "--gpus";
    if (sharded && !o.describe && !o.order_sharded && (!o.order_fields.empty() || o.limit > 0)) {
        std::fprintf(stderr, "vdlrun: --order-by / --limit are not served with --gpus: the ranks hold disjoint result rows and the merge of per-rank "
                             "top-N results is not built; run the ordered query on one GPU\n");
        return 3;
    }
    {
        // wide sums with --gpus: only with the wide merge switched on -- refused here, before any rank starts, in the words of the entry point
        const char *we = std::getenv("VDL_WIDE_SUMS"), *se = std::getenv("VDL_WIDE_SHARDED");
        const bool wide_on = o.wide > 0 || (o.wide < 0 && we && (!std::strcmp(we, "1") || !std::strcmp(we, "2")));
        const bool merge_on = o.wide_sharded || (se && !std::strcmp(se, "1"));
        if (sharded && !o.describe && wide_on && !merge_on) {
            std::fprintf(stderr, "vdlrun: --wide-sums / --checked-sums are not served with --gpus unless --wide-sharded is given: wide sums are on for this plan "
                                 "(vdl_plan_set_wide_sums), and the sharded routes merge the ranks' partial words with 64-bit operators (the merge has no "
                                 "add-with-carry); add --wide-sharded, or run it on one GPU\n");
            return 3;
        }
    }
    if (o.batch_sharded && (!sharded || o.batch_files.empty() || !o.jit)) {
        std::fprintf(stderr, "usage: vdlrun --batch-sharded needs --gpus N, --batch FILE and --jit or --jit-tune: it runs the programs as one vdl_run_batch_sharded on every rank\n");
        return 2;
    }
    if (sharded && !o.describe && !o.batch_files.empty() && !o.batch_sharded) {
        std::fprintf(stderr, "vdlrun: --batch is not served with --gpus: a sharded run takes one plan; run the batch on one GPU\n");
        return 3;
    }
    for (const std::string &path : o.batch_files) {
        std::ifstream f(path, std::ios::binary);
        if (!f) { std::fprintf(stderr, "vdlrun: cannot read %s\n", path.c_str()); return 1; }
        o.batch_texts.push_back(std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>()));
    }
    if (!sharded || o.describe) {
        Reply r;
        std::vector<Reply> more;
        const int rc = run_rank(o, text, 0, 1, "", r, &more);
        if (rc == 0 && !o.describe) { print_reply(r); for (const Reply &m : more) print_reply(m); }
        return rc;
    }
    // one process per GPU, forked before anything in this process has touched HIP (no HIP call above this line)
    char tmpl[] = "/tmp/vdlrun.XXXXXX";
    const char *dir = mkdtemp(tmpl);
    if (!dir) { std::perror("vdlrun: mkdtemp"); return 1; }
    std::vector<pid_t> kids;
    for (int r = 0; r < o.gpus; r++) {
        const pid_t pid = fork();
        if (pid < 0) { std::perror("vdlrun: fork"); return 1; }
        if (pid == 0) {
            dup2(2, 1);                                      // stdout carries the parent's reply only (RCCL prints a banner at start-up)
            Reply mine;
            std::vector<Reply> more;
            int rc = run_rank(o, text, r, o.gpus, dir, mine, &more);
            if (rc == 0 && !write_reply(std::string(dir) + "/out." + std::to_string(r), mine)) rc = 1;
            for (size_t k = 0; k < more.size() && rc == 0 && r == 0; k++)       // (--batch-sharded: rank 0's further replies are the ones printed)
                if (!write_reply(std::string(dir) + "/out.0." + std::to_string(k + 1), more[k])) rc = 1;
            std::fflush(nullptr);
            _exit(rc);
        }
        kids.push_back(pid);
    }
    // a rank that fails leaves its peers waiting in the communicator: the first failure ends the others
    int failed = 0;
    for (size_t left = kids.size(); left > 0; left--) {
        int st = 0;
        const pid_t pid = waitpid(-1, &st, 0);
        if (pid < 0) { failed++; break; }
        if (!WIFEXITED(st) || WEXITSTATUS(st) != 0) {
            if (!failed)
                for (pid_t other : kids) if (other != pid) kill(other, SIGTERM);
            failed++;
        }
    }
    Reply all;
    for (int r = 0; r < o.gpus && !failed; r++) {
        Reply part;
        if (!read_reply(std::string(dir) + "/out." + std::to_string(r), part)) { failed++; break; }
        if (r == 0) { all = part; continue; }
        if (part.replicated) continue;                       // fold plans: every rank printed the same answer
        for (size_t k = 0; k < all.outs.size() && k < part.outs.size(); k++) {
            all.outs[k].vals.insert(all.outs[k].vals.end(), part.outs[k].vals.begin(), part.outs[k].vals.end());
            all.outs[k].hi.insert(all.outs[k].hi.end(), part.outs[k].hi.begin(), part.outs[k].hi.end());
        }
    }
    std::vector<Reply> more(o.batch_sharded ? o.batch_texts.size() : 0);
    for (size_t k = 0; k < more.size(); k++) {
        const std::string path = std::string(dir) + "/out.0." + std::to_string(k + 1);
        if (!failed && !read_reply(path, more[k])) failed++;
        std::remove(path.c_str());
    }
    for (int r = 0; r < o.gpus; r++) std::remove((std::string(dir) + "/out." + std::to_string(r)).c_str());
    std::remove((std::string(dir) + "/id").c_str());
    rmdir(dir);
    if (failed) { std::fprintf(stderr, "vdlrun: %d rank(s) failed\n", failed); return 1; }
    print_reply(all);
    for (const Reply &m : more) print_reply(m);
    return 0;
}
