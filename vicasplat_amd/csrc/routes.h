// Which kernels a forward GEMM / 3x3 convolution / attention call reaches: pure functions of integers and booleans, no HIP.  gemm.hip,
// conv.hip, attention.hip and attention_bwd.hip launch what these return; tests/test_routes_cpu.py compiles them on the host
// (tests/route_probe.cpp) and compares them with tests/gemm_f64.py plan(), the pinned shapes of the convolution and attention routes, the
// route every case of tests/attention_route_cases.py names, and the thresholds model/encoder/heads/dpt.py repeats.
#pragma once
#include <cstdint>

// for xcd_remap, the one function here that kernels call too
#ifdef __HIPCC__
#define VS_HOST_DEVICE __host__ __device__
#else
#define VS_HOST_DEVICE
#endif

namespace vs {
namespace route {

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline long long cdiv64(long long a, long long b) { return (a + b - 1) / b; }

// XCD-aware workgroup order.  The hardware deals consecutive workgroup ids to consecutive XCDs (8 on
// MI355X, each with its own L2): ids b, b + 8, b + 16 .. share one.  This maps id `bid` of a grid of n to a LOGICAL id so that each XCD gets one
// contiguous range of them (the first n % 8 XCDs one more than the rest) and neighbouring logical ids meet in one L2.  A permutation of [0, n)
// for every n >= 1: tests/test_routes_cpu.py.
VS_HOST_DEVICE inline int xcd_remap(int bid, int n) {
    const int q = n / 8, r = n % 8, xcd = bid % 8, idx = bid / 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// ---- forward GEMM.  Classes as the kernels' template argument (gemm_common.h): 0 f16, 1 bf16, 2 f32 MFMA, 3 split; K2 counts 2-byte units. ----
constexpr int kF32 = 2, kSplit = 3;
enum class Leaf { SmallM, Skinny, G256, Mi2, Mi4, Mi8 };
struct GemmStep { Leaf leaf; int nw, mf, m_lo, m_hi, ksplit; };      // rows [m_lo, m_hi); nw / mf: waves and row fragments of the weight-streaming kernel
struct GemmPlan { int n; GemmStep step[2]; };

// weight-streaming kernel: 16 waves split K when it is long (each walks <= 8 k-steps of 4096), 8 otherwise; 1 or 4 row fragments
inline GemmStep smallm_step(int m_lo, int m_hi, int K2) {
    const bool one = m_hi - m_lo <= 16, deep = K2 / 32 >= 64;
    return {Leaf::SmallM, deep ? 16 : 8, one ? 1 : 4, m_lo, m_hi, 1};
}
inline bool smallm_takes(int cls, int rows, int epi, bool a_packed, bool out_packed) {
    return rows <= 64 && epi != 4 && epi != 5 && !out_packed && (cls == kSplit || !a_packed);
}

// skinny kernel (<= 256 rows).  Epilogue 2 with the residual already in `out`: split K over workgroups while the grid is small and a
// slice keeps >= 8 blocks per wave
inline GemmStep skinny_step(int m_lo, int m_hi, int N, int K2, int epi, bool resid, bool deterministic) {
    const int gy = cdiv(m_hi - m_lo, 64), gx = cdiv(N, 64);
    int ks = 1;
    if (epi == 2 && !resid && !deterministic)
        while (ks < 8 && gx * gy * ks * 2 <= 384 && K2 / 64 / (ks * 2) >= 32) ks *= 2;
    return {Leaf::Skinny, 0, 0, m_lo, m_hi, ks};
}
inline bool skinny_takes(int cls, int rows, int K2, bool a_packed, bool out_packed) {
    return rows <= 256 && K2 % 64 == 0 && (cls == kSplit || (!a_packed && !out_packed));
}

// Rows [M - rem, M) of a tiled GEMM: 65 .. 256 rows on the skinny kernel (and fewer where the weight-streaming kernel lacks the epilogue:
// RoPE pairs columns 16 apart, a packed output is written in 32-column blocks), <= 64 on the weight-streaming kernel, else one row of
// 128 x 128 tiles.  Such a tail is a handful of tiles walking all of K serially: for the f32 residual epilogue it splits K over up to 8
// workgroups per tile (>= 8 k-steps each) and the partial sums meet through f32 atomics in `out`, which must already hold the residual.
// (Measured and not kept: the 192-row tails of the bench step on the weight-streaming kernel, 246.6 / 248.3 vs 247.6 / 247.7 ms per step.)
inline GemmStep tail_step(int cls, int M, int rem, int N, int K2, int epi, bool resid, bool a_packed, bool out_packed, bool deterministic) {
    int ks = 1;
    if (epi == 2 && rem > 64 && !resid && !deterministic) {
        const int tiles = cdiv(rem, 128) * cdiv(N, 128);
        while (ks < 8 && (K2 / 32) % (ks * 2) == 0 && K2 / 32 / (ks * 2) >= 8 && tiles * ks * 2 <= 512) ks *= 2;
    }
    if (skinny_takes(cls, rem, K2, a_packed, out_packed) && (rem > 64 || epi == 4 || epi == 5 || out_packed))
        return skinny_step(M - rem, M, N, K2, epi, resid, deterministic);
    if (smallm_takes(cls, rem, epi, a_packed, out_packed)) return smallm_step(M - rem, M, K2);
    return {Leaf::Mi4, 0, 0, M - rem, M, ks};
}

inline GemmPlan gemm_plan(int cls, int M, int N, int K2, int epi, bool resid, bool a_packed, bool out_packed, bool deterministic) {
    auto one = [&](Leaf leaf) { return GemmPlan{1, {{leaf, 0, 0, 0, M, 1}, {}}}; };
    auto with_tail = [&](Leaf leaf, int rem) {
        return GemmPlan{2, {{leaf, 0, 0, 0, M - rem, 1}, tail_step(cls, M, rem, N, K2, epi, resid, a_packed, out_packed, deterministic)}};
    };
    // reference-precision class (exact f32 MFMA at 1/16 of the 16-bit rate): the matrix pipe, not the tile schedule, sets the time, so
    // one route per shape class and no tail: 256x256 tiles when K allows (128 units = 64 floats), 128x128 otherwise
    if (cls == kF32) {
        if (M <= 64 && epi != 4) return GemmPlan{1, {smallm_step(0, M, K2), {}}};
        return one(K2 % 128 == 0 ? Leaf::G256 : Leaf::Mi4);
    }
    if (smallm_takes(cls, M, epi, a_packed, out_packed)) return GemmPlan{1, {smallm_step(0, M, K2), {}}};
    if (skinny_takes(cls, M, K2, a_packed, out_packed)) return GemmPlan{1, {skinny_step(0, M, N, K2, epi, resid, deterministic), {}}};
    // 256x256 tiles run one 8-wave workgroup per CU, i.e. in rounds of 256 tiles, and a partly filled round costs as much
    // as a full one (M = frames * 257 tokens never divides).  So the big tiles only get as many rows as fill whole rounds;
    // the remaining rows are finished by a tail launch -- a short round instead of a mostly idle long one.
    if (K2 % 128 == 0 && M >= 256) {
        const int tn = cdiv(N, 256), mt = M / 256;
        const long long full = (long long)mt * tn, rounds_all = (cdiv(M, 256) * (long long)tn + 255) / 256;
        int mt_main = mt;
        if (full > 256 && full % 256 != 0) mt_main = (int)((full / 256) * 256 / tn);  // whole rounds only
        const int rem = M - mt_main * 256;
        // cost in units of one 256x256 round; a 128x128 round (768 tiles) is about 0.31 of it
        const long long tiles4 = (long long)cdiv(rem, 128) * cdiv(N, 128);
        const double cost_split = (double)(((long long)mt_main * tn + 255) / 256) + (rem > 0 ? 0.31 * (double)((tiles4 + 767) / 768) : 0.0);
        const long long tiles_one = cdiv(M, 256) * (long long)tn;
        // a last round that is >= 95 % full is not worth a second launch (e.g. 31 eight-view scenes: 249 row tiles -> 3.89 / 11.67 /
        // 15.56 rounds): one launch, no tail
        const bool nearly_full = tiles_one * 100 >= rounds_all * 256 * 95;
        if (!nearly_full && rem > 0 && mt_main > 0 && cost_split < (double)rounds_all - 0.05) return with_tail(Leaf::G256, rem);
        // (a round that is >= 70 % full still beats the 256x128 tiles: 8 scenes x 257 tokens x 768 columns = 195 tiles, 385 vs 391 ms per
        // split-class training step)
        if (tiles_one * 100 >= rounds_all * 256 * 70) return one(Leaf::G256);
    }
    // 256x128 tiles (half the W-panel traffic and LDS-DMA issue per flop of 128x128) whenever there are enough of them
    // to fill 256 CUs x 2 resident workgroups; 128x128 otherwise.
    const int tiles_n = cdiv(N, 128);
    const long long t8 = (long long)cdiv(M, 256) * tiles_n;
    const int mi = t8 >= 256 ? 8 : 4, bm = 32 * mi, slots = 256 * (mi == 8 ? 2 : 3);
    const int rem = M % bm;
    const long long full = (long long)(M / bm) * tiles_n;
    // a partly filled extra round costs a whole one.  The matrix pipes of a CU are shared by its resident workgroups, so a "round"
    // of MFMA-bound tiles is 256 tiles (one per CU), not `slots` -- one 8-view scene's fc1 (2 056 rows x 4 096 columns) is 288 tiles of
    // 256 x 128, i.e. TWO rounds with the second 12 % full; peeling the 8 leftover rows makes it one (110 -> 70 us).
    const bool split = full > 0 && rem > 0 && rem <= bm / 2 &&
                       ((full + tiles_n + slots - 1) / slots > (full + slots - 1) / slots || (full + tiles_n + 255) / 256 > (full + 255) / 256);
    const int m_main = split ? M - rem : M;
    Leaf leaf = mi == 8 ? Leaf::Mi8 : Leaf::Mi4;
    // small batches (one 8-view scene = 2 056 rows): the residual epilogue's GEMMs (attention projection, fc2: N = 1024 / 768) are
    // 136 / 102 tiles of 128 x 128 -- half the chip for one pass over K.  64-row tiles (MI = 2: the same kernel) double the workgroups.
    // (Measured and not kept: cutting K over blockIdx.y for them instead -- the epilogue's atomic traffic costs more than the idle CUs:
    // B = 1 encoder 22.2 -> 26.2 ms, B = 2 29.7 -> 35.3 ms.)
    if (cls == kSplit && mi == 4 && epi == 2 && (long long)cdiv(m_main, 128) * tiles_n <= 192 && m_main > 64) leaf = Leaf::Mi2;
    return split ? with_tail(leaf, rem) : one(leaf);
}

// ---- 3x3 convolution (conv.hip).  dtype as the ABI: 1 f16, 2 bf16, 3 f32, 4 split; Cin2 counts 2-byte units per pixel. ----
// K-tiles (64 units) per tap as a shift, for the kernels that need a power of two: Cin2 in {64, 128, 256, 512}; -1 otherwise.
inline int conv_cshift(int Cin2) {
    for (int sft = 0; sft < 4; ++sft)
        if (Cin2 == (64 << sft)) return sft;
    return -1;
}
// the "+ 16" of a relu flag (split class): the input is the packed (hi, lo) image.  Returns it and clears it from the flag.
inline int take_packed_flag(int32_t &flag) {
    const int packed = (flag & 16) ? 1 : 0;
    flag &= ~16;
    return packed;
}

enum class ConvKind { Halo256, Tile256, Tile256x128, Wave4, PackedNotTaken };
struct ConvRoute { ConvKind kind; int kpt, mi; long long grid; };    // kpt: K-tiles per tap (tile kernels); mi: 32-row fragments per block (4-wave kernel)

inline ConvRoute conv3x3_route(int dtype, long long M, int H, int W, int Cin2, int Cout, int stride, bool a_packed) {
    const int cshift = conv_cshift(Cin2);
    // the 256 x 256 tile kernel takes a power-of-two Cin in every class and, in the split class with a plain f32 input, any Cin that is a
    // whole number of 64-unit K-tiles per tap (96 -> 128, 192, 384, 768 channels of the DPT reassemble / layer_rn convolutions)
    const int kpt_any = (Cin2 % 64 == 0 && Cin2 / 64 <= 64) ? Cin2 / 64 : -1;
    const int kpt = cshift >= 0 ? 1 << cshift : (dtype == 4 && !a_packed ? kpt_any : -1);
    const long long t256 = cdiv64(M, 256) * cdiv(Cout, 256);
    // >= 150 tiles in the split class: a 59 %-full round of 256 x 256 tiles beats the 4-wave kernel's one and a half rounds at two workgroups
    // per CU (16 x 16 maps of the bench step: 0.21 -> 0.17 ms per convolution); 8 x 8 maps (48 tiles) stay where they were
    const long long t256_min = dtype == 4 ? 150 : 224;
    if (kpt > 0 && Cout % 256 == 0 && (9 * kpt) % 2 == 0 && t256 >= t256_min) {
        // the halo-tile body (conv3x3_256_halo_split_kernel) for the shapes it covers; M / 256 tiles either way
        const bool halo = dtype == 4 && stride == 1 && Cout == 256 && H % 16 == 0 && W % 16 == 0 && !a_packed && (long long)H * W * Cin2 < 2147483647LL;
        return {halo ? ConvKind::Halo256 : ConvKind::Tile256, kpt, 0, t256};
    }
    const long long big = cdiv64(M, 256) * cdiv(Cout, 128), t4 = cdiv64(M, 128) * cdiv(Cout, 128);
    if (dtype == 3) return {ConvKind::Wave4, 0, 4, t4};
    if (dtype != 4) return big >= 256 ? ConvRoute{ConvKind::Wave4, 0, 8, big} : ConvRoute{ConvKind::Wave4, 0, 4, t4};
    // 224 tiles: tests/test_routes_cpu.py holds PACKED_CONV_MIN_PIXELS of model/encoder/heads/dpt.py to it.  (Cout = 256 maps too small for the
    // 256 x 256 kernel: the 4-wave kernel is 8 % faster there, measured)
    if (cshift >= 0 && Cout % 128 == 0 && Cout % 256 != 0 && (9 * kpt) % 2 == 0 && big >= 224)
        return {ConvKind::Tile256x128, kpt, 0, cdiv64(M, 256) * (Cout / 128)};
    if (a_packed) return {ConvKind::PackedNotTaken, 0, 0, 0};        // only the tile kernels read a packed input
    // small batches (one 8-view scene: 16 x 16 / 32 x 32 maps = 32 / 128 tiles of 128 x 128 for 256 CUs): 64-row tiles (MI = 2) double the workgroups
    if (big >= 512) return {ConvKind::Wave4, 0, 8, big};
    if (t4 <= 192 && M > 64) return {ConvKind::Wave4, 0, 2, cdiv64(M, 64) * cdiv(Cout, 128)};
    return {ConvKind::Wave4, 0, 4, t4};
}

// ---- attention (attention.hip, attention_bwd.hip).  dtype as the ABI after its packing bits are taken off: 1 f16, 2 bf16, 3 f32, 4 split. ----
// The resident kernel holds all keys of a (batch, head) in LDS (its staging rounds are sized by kResMaxKeys) and walks 3 x 8 groups of 16 queries.
constexpr int kResMaxKeys = 320, kResMaxQueries = 3 * 8 * 16;
enum class AttnKind { Res, Tile64, Tile128, F32, Split64, Split128, Packed96 };
struct AttnRoute { AttnKind kind; long long gx; int gy, gz, block; };    // grid (gx, gy, gz); Packed96's is linear: gx = tiles * H * nbatch

inline AttnRoute attention_route(int dtype, bool in_packed, int nbatch, int H, int Lq, int Lk, bool has_seg, bool has_len) {
    if (dtype == 4 && in_packed) return {AttnKind::Packed96, (long long)cdiv(Lq, 96) * H * nbatch, 1, 1, 256};
    if (dtype == 3) return {AttnKind::F32, cdiv(Lq, 64), H, nbatch, 256};
    if (dtype != 4 && !has_seg && !has_len && Lk <= kResMaxKeys && Lq <= kResMaxQueries) return {AttnKind::Res, 1, H, nbatch, 512};
    // Lk as the entry receives it.  Every caller of this project passes Lk = 0 with key segments (the lengths are in kv_seg), so Lk_eff is 0
    // there and a segmented call always takes the 64-query kernels.
    const int Lk_eff = has_seg ? 2 * Lk : Lk;
    // 128 queries per workgroup (more MFMAs per staged K / V tile) when that still leaves >= 2 workgroups per CU, and only for long key
    // lists: the 257 / 516-key shapes are latency bound and run faster with 64-query workgroups at higher occupancy
    const bool big = (long long)cdiv(Lq, 128) * H * nbatch >= 512 && Lk_eff > (dtype == 4 ? 256 : 1024);
    const AttnKind kind = dtype == 4 ? (big ? AttnKind::Split128 : AttnKind::Split64) : (big ? AttnKind::Tile128 : AttnKind::Tile64);
    return {kind, cdiv(Lq, big ? 128 : 64), H, nbatch, 256};
}

// backward: x-extent of the dq and the dk|dv grids (times H x nbatch); `keys` bounds the key list of every batch item.  16-bit: two 16-row
// groups per wave in both kernels; split: two for dq, one for dk|dv (two key groups spill, attention_bwd.hip)
struct AttnBwdRoute { int keys, gq, gk; };
inline AttnBwdRoute attention_bwd_route(bool split, int Lq, int Lk, bool has_seg, int max_keys) {
    const int keys = has_seg ? max_keys : Lk;
    return {keys, cdiv(Lq, 128), cdiv(keys, split ? 64 : 128)};
}

}  // namespace route
}  // namespace vs
