// vdl_column_image.h -- frame-of-reference images of catalog columns: the rules only (pure functions, no device, no context;
// tests/test_column_images_cpu.py checks them against brute force under ASan + UBSan).  Used by vdl_engine.cpp.
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

// Uses of a column inside one aggregate scan (bit masks over the scan's columns), gathered by the binder: an affine image may be
// read only when every use is a range filter, a formula test or an aggregate factor (other than a FIRST); a pure narrowing always.
inline bool usable(const Image &im, bool raw_use) { return im.width > 0 && (im.pure() || !raw_use); }

// Uses of a column inside a scan with derived columns -- a fused front, a dimension scan, a semi-join scan.  A column whose values the
// select pass needs only for its filters and formula tests stays in the encoded domain there (bounds rewritten as above).  A column
// whose values it needs per row -- the source of a lookup or a difference, the position of a semi-join -- is decoded with the tile,
// and that may only cost an add: such a column is read from its image only when the scale is 1 (its filters stay as planned).  The
// take side of a front decodes whatever it loads for a survivor, base + scale * e in wrapping 64-bit arithmetic (outputs, operands of
// row expressions), once per survivor, at any scale; a carried column travels decoded, or is not carried.  A pure narrowing decodes
// to itself and costs nothing.
inline bool usable_in_vscan(const Image &im, bool per_row_value) { return im.width > 0 && (im.scale == 1 || !per_row_value); }
// the kernels must decode the column's values (MsArgs::decode)
inline bool needs_decode(const Image &im) { return im.width > 0 && !im.pure(); }

}  // namespace img
}  // namespace vdl
