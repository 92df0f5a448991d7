// vdl_column_image.h -- frame-of-reference images of catalog columns: the rules only (pure functions, no device, no context;
// tests/test_column_images_cpu.py checks them against brute force under ASan + UBSan).  Used by vdl_bind.cpp.
//
// A column whose values span few significant digits is kept a second time, narrow: v = base + scale * e with e stored in 1, 2 or
// 4 bytes.  An aggregate scan reads the image instead of the column where every use of the column there can be rewritten into the
// encoded domain: a range filter [lo, hi] becomes a range of e, an aggregate factor (a + s * v) becomes (a + s * base) + (s * scale) * e
// (exact mod 2^64, which is how the kernels compute: the sums stay bit-identical).  A pure narrowing (base 0, scale 1) holds the
// very values and may stand in for the column anywhere.
#pragma once
#include <cstdint>

namespace vdl {
namespace img {

struct Image {
    int width = 0;                 // 1, 2 or 4 bytes; 0 = no image
    int64_t base = 0, scale = 1;   // v = base + scale * e
    bool pure() const { return base == 0 && scale == 1; }
};

inline int64_t width_min(int w) { return w >= 8 ? INT64_MIN : -((int64_t)1 << (8 * w - 1)); }
inline int64_t width_max(int w) { return w >= 8 ? INT64_MAX : ((int64_t)1 << (8 * w - 1)) - 1; }

// the narrowest of 1, 2, 4 bytes that holds [lo, hi] as signed values; 8 when none does
inline int narrowest(int64_t lo, int64_t hi) {
    for (int w : {1, 2, 4}) if (lo >= width_min(w) && hi <= width_max(w)) return w;
    return 8;
}

// 10^p for p in 0..18
inline int64_t pow10(int p) {
    int64_t x = 1;
    for (int i = 0; i < p; i++) x *= 10;
    return x;
}

// The image of a column of `stored` bytes whose values lie in [mn, max] and all differ from each other by multiples of 10^p
// (p <= 18: larger is taken as 18): a pure narrowing when that is as narrow as the affine form, else base = mn, scale = 10^p.
// width 0: no image (it would not be narrower than the column, or max - mn does not fit int64).
inline Image choose(int stored, int64_t mn, int64_t mx, int p) {
    Image im;
    if (mn > mx || stored <= 1) return im;
    if (p < 0) p = 0;
    if (p > 18) p = 18;
    const int pure_w = narrowest(mn, mx);
    const unsigned __int128 span = (unsigned __int128)((__int128)mx - (__int128)mn);
    int aff_w = 8;
    if (span <= (unsigned __int128)INT64_MAX) {
        const int64_t scale = pow10(p);
        aff_w = narrowest(0, (int64_t)(span / (unsigned __int128)scale));
        if (aff_w < pure_w) { im.base = mn; im.scale = scale; }
    }
    const int w = pure_w <= aff_w ? pure_w : aff_w;
    if (w >= stored) return Image{};
    im.width = w;
    if (pure_w <= aff_w) { im.base = 0; im.scale = 1; }
    return im;
}

// floor / ceil of x / d for d > 0
inline __int128 floor_div(__int128 x, __int128 d) { __int128 q = x / d; if ((x % d) != 0 && x < 0) q--; return q; }
inline __int128 ceil_div(__int128 x, __int128 d) { __int128 q = x / d; if ((x % d) != 0 && x > 0) q++; return q; }

// The filter lo <= v <= hi as a filter on e.  The unfiltered sentinels (INT64_MIN, INT64_MAX) stay as they are; every other range
// is clamped to what the image's width can hold, and a range that holds no encoded value becomes [1, 0] (nothing passes).
inline void map_range(const Image &im, int64_t lo, int64_t hi, int64_t *elo, int64_t *ehi) {
    if (lo == INT64_MIN && hi == INT64_MAX) { *elo = lo; *ehi = hi; return; }
    const __int128 wlo = width_min(im.width), whi = width_max(im.width);
    __int128 a = ceil_div((__int128)lo - im.base, im.scale), b = floor_div((__int128)hi - im.base, im.scale);
    if (a < wlo) a = wlo;
    if (b > whi) b = whi;
    if (a > b) { *elo = 1; *ehi = 0; return; }
    *elo = (int64_t)a; *ehi = (int64_t)b;
}

// The factor a + s * v over the image: a' + s' * e with a' = a + s * base, s' = s * scale, in wrapping 64-bit arithmetic
inline void compose(const Image &im, int64_t a, int64_t s, int64_t *a2, int64_t *s2) {
    *a2 = (int64_t)((uint64_t)a + (uint64_t)s * (uint64_t)im.base);
    *s2 = (int64_t)((uint64_t)s * (uint64_t)im.scale);
}
// the factor is the bare value (MAggDesc::plain)
inline bool plain(int64_t a, int64_t s) { return a == 0 && s == 1; }

// ---- the use rules ---------------------------------------------------------------------------------------------------------
// What a scan does with the image of a column it reads -- a streamed table column, or the target of a lookup (VC_GATHER: dimension
// column `name` at row v[idx]; its image read in its place is a lookup image, with as many entries as the column, the index checked
// against the row count as before).  The rules speak of the use of the VALUE, streamed or looked up, so one statement serves both
// (tests/test_lookup_images_cpu.py checks them against brute force; the kernel headers' comments call use_in_vscan "usable_in_vscan"):
enum Use { USE_CATALOG = 0,      // not readable here: the catalog column
           USE_ENCODED = 1,      // read and left encoded: bounds and formula tests through map_range, factors through compose
           USE_DECODED = 2 };    // read and decoded where it is loaded (MsArgs::decode): bounds and tests as planned
// In an aggregate scan, which cannot decode with the tile.  raw_use: the scan needs the stored value itself -- the source of a
// derived column other than a formula test, a load of the group key, the column of a FIRST aggregate.  An affine image may be read
// only when every use is a range filter, a formula test or an aggregate factor; a pure narrowing always, and its encoded values are
// the column's: never decoded.
inline Use use_in_aggregate(const Image &im, bool raw_use) { return im.width > 0 && (im.pure() || !raw_use) ? USE_ENCODED : USE_CATALOG; }
// In a scan with derived columns -- a fused front, a dimension scan, a semi-join scan.  A value the select pass needs only for its
// filters and formula tests stays in the encoded domain there (bounds rewritten as above).  A value it needs per row -- the source of
// a lookup or a difference, the position of a semi-join -- is decoded as it is loaded, and that may only cost an add: it is read from
// the image only when the scale is 1 (its filters stay as planned).  A pure narrowing decodes to itself and costs nothing.  (The take
// side of a front reads what these rules let the select side read and decodes whatever it loads for a survivor, base + scale * e in
// wrapping 64-bit arithmetic, once per survivor, at any scale; a carried column travels decoded, or is not carried.)
inline Use use_in_vscan(const Image &im, bool per_row_value) {
    if (im.width <= 0 || (im.scale != 1 && per_row_value)) return USE_CATALOG;
    return per_row_value && !im.pure() ? USE_DECODED : USE_ENCODED;
}

// ---- bit-packed images ---------------------------------------------------------------------------------------------------
// A column's byte image (base, scale, e) is kept a third time with e' = e - emin in exactly `bits` bits per row, bits = the bit
// length of emax - emin (1 for a constant column): v = base' + scale * e' with base' = base + scale * emin (wrapping).  Built only
// when it is narrower than the byte image.  Layout: lane-transposed stripes of 2048 rows (64 lanes x 32 values): row
// 2048 s + 64 j + l is value j of lane l in stripe s; lane l's 32 values are a bit stream of `bits` dwords (value j in bits
// [j bits, (j + 1) bits), possibly across two dwords), and dword k of lane l in stripe s lies at dword (s bits + k) 64 + l.  The
// image is padded with zeros to whole stripes.  A wave that reads dword k of a stripe reads 256 contiguous bytes.
constexpr int kStripeLanes = 64, kStripeValues = 32, kStripeRows = kStripeLanes * kStripeValues;
struct Packed {
    int bits = 0;                  // 1..32; 0 = no packed image
    int64_t base = 0, scale = 1;   // v = base + scale * e'
};

// bit length of x; 1 for 0
inline int bit_length(uint64_t x) {
    int b = 1;
    while (b < 64 && (x >> b) != 0) b++;
    return b;
}

// the packed image of a byte image `im` whose encoded values lie in [emin, emax]; bits 0 when it would not be narrower
inline Packed pack(const Image &im, int64_t emin, int64_t emax) {
    Packed pk;
    if (im.width <= 0 || emin > emax) return pk;
    const int bits = bit_length((uint64_t)emax - (uint64_t)emin);
    if (bits > 32 || bits >= 8 * im.width) return pk;
    pk.bits = bits;
    pk.base = (int64_t)((uint64_t)im.base + (uint64_t)im.scale * (uint64_t)emin);
    pk.scale = im.scale;
    return pk;
}

inline int64_t stripes(int64_t n) { return (n + kStripeRows - 1) / kStripeRows; }
// dwords of a packed image of n rows (padded to whole stripes)
inline int64_t packed_dwords(int64_t n, int bits) { return stripes(n) * bits * kStripeLanes; }
// where row i's value starts: the dword index of its first bit and the bit inside it
inline void packed_at(int64_t i, int bits, int64_t *dword, int *bit) {
    const int64_t s = i / kStripeRows, j = (i % kStripeRows) / kStripeLanes, l = i % kStripeLanes;
    const int64_t o = j * bits;
    *dword = (s * bits + o / 32) * kStripeLanes + l;
    *bit = (int)(o % 32);
}

// The filter lo <= v <= hi as a filter on e' in [0, 2^bits - 1]: the unfiltered sentinels stay, every other range is clamped to
// that domain, and a range that holds no stored value becomes [1, 0] (as map_range).
inline void map_range_packed(const Packed &pk, int64_t lo, int64_t hi, int64_t *plo, int64_t *phi) {
    if (lo == INT64_MIN && hi == INT64_MAX) { *plo = lo; *phi = hi; return; }
    const __int128 top = ((__int128)1 << pk.bits) - 1;
    __int128 a = ceil_div((__int128)lo - pk.base, pk.scale), b = floor_div((__int128)hi - pk.base, pk.scale);
    if (a < 0) a = 0;
    if (b > top) b = top;
    if (a > b) { *plo = 1; *phi = 0; return; }
    *plo = (int64_t)a; *phi = (int64_t)b;
}
// the factor a + s * v over the packed image, as compose
inline void compose_packed(const Packed &pk, int64_t a, int64_t s, int64_t *a2, int64_t *s2) {
    Image im;
    im.width = 4; im.base = pk.base; im.scale = pk.scale;
    compose(im, a, s, a2, s2);
}

// ---- step images ---------------------------------------------------------------------------------------------------------
// A column that never decreases and whose consecutive rows differ by 0 or 1 -- the join index of a table clustered by its parent:
// lineitem by order -- is fully described by its first value, one bit per row ("this row starts a new parent") and one anchor per
// 64 rows.  With G = ceil(n / 64) groups:
//   heads[g]  (uint64)  bit i is 1 iff row r = 64 g + i has r >= 1 and v[r] != v[r - 1]
//   anchor[g] (uint32)  v[64 g - 1] - base for g >= 1, anchor[0] = 0              (base = v[0])
//   v[r] = base + anchor[r >> 6] + popcount(heads[r >> 6] & (~0 >> (63 - (r & 63))))
// 12 bytes per 64 rows.  Both arrays are padded to whole tiles of the projection scans (`tile` rows, a multiple of 64: a tile load
// never runs off the end) with head words 0 and anchors v[n - 1] - base: rows past n decode to v[n - 1].  The anchors follow the
// padded head words in one buffer.  1 <= n < 2^32, so that every anchor fits its 32 bits.  Read by the scans with derived columns
// (fused fronts, dimension scans, semi-join scans), which decode it with the tile: always to the column's own values.
constexpr int kStepGroup = 64;
struct Steps {
    bool present = false;
    int64_t base = 0;
};
inline bool steps_rows_ok(int64_t n) { return n >= 1 && n < ((int64_t)1 << 32); }
inline int64_t step_groups(int64_t n) { return (n + kStepGroup - 1) / kStepGroup; }

}  // namespace img
}  // namespace vdl
