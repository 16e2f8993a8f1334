// The forward of a view, per Gaussian: fused preprocess (project! + spherical_harmonics! + tile rect + per-tile occupancy
// count and binning), and the same kernel's SCATTER form, the second pass of the compact binning mode.
//
// Reference behaviour: src/rasterization/projection.jl:39-130, 259-287, spherical_harmonics.jl:1-74, utils.jl:14-29,
// 85-142, render.jl:288-420.
//
// This translation unit is compiled with -ffp-contract=off: every fp32 expression is evaluated as written (no FMA), so
// the discrete outputs (radii, tile rects) and the per-Gaussian floats are bit-reproducible against the CPU oracle.  The
// kernel is HBM-bound (192 B of SH per Gaussian), the extra VALU ops are free.
//
// bench.py's hashes of the kernel sources, which mark profiles/pmc_traffic.json stale, cover pergauss.hip and not this
// file: after a change here, run tools/measure_pmc.sh again.
#include "gsr_kernels.h"
#include "gsr_dispatch.h"
#include "tile_mask.h"
#include "wave_reduce.h"
#include "agg_plan.h"
#include "splat_math.h"

namespace {
using namespace gsr::splat;

constexpr uint32_t EMIT_COOP = 48;  // tiles per rect above which the wave emits cooperatively
constexpr int kAggThreads = gsr_agg::kThreads;  // workgroup of preprocess_kernel's aggregating form (agg_plan.h: shared with the policy layer)
// Gradient-row slots of a Gaussian (Gaussian-major, gsr_kernels.h): rects of at most DENSE_RECT tiles get one slot per
// EMITTED tile — preprocess keeps the bit mask of the rect's tiles that passed the footprint test in the record, the
// sort's emit ranks a tile by a popcount below its bit, the per-Gaussian backward sums popcount(mask) contiguous rows
// without repeating the tests.  Larger rects keep one slot per tile of the rect (the culled ones are never written or
// read).  Exact culling drops 31 % of config 3's instances: the row buffer and its read in pergauss_bwd shrink with it.
constexpr uint32_t DENSE_RECT = GSR_DENSE_RECT;

// utils.jl:14-29 get_rect; float ceil-div as gpu_cld
__device__ __forceinline__ void get_rect(float mx, float my, int radius, int gx, int gy, int rmin[2], int rmax[2]) {
    const float px[2] = {mx, my};
    const int grid[2] = {gx, gy};
#pragma unroll
    for (int k = 0; k < 2; k++) {
        float lo = floorf((px[k] - (float)radius) / 16.0f);
        float hi_arg = (px[k] + (float)radius) + 16.0f - 1.0f;
        float hi = floorf(hi_arg / 16.0f);
        int ilo = (int)lo, ihi = (int)hi;
        rmin[k] = ilo < 0 ? 0 : (ilo > grid[k] ? grid[k] : ilo);
        rmax[k] = ihi < 0 ? 0 : (ihi > grid[k] ? grid[k] : ihi);
    }
}

// ---------------------------------------------------------------------------------
// The FLATTENED walk of preprocess_kernel's binning (both forms).  In scene order a wave's slowest lane has 13.6 pair
// requests at config 3 and the average lane 3.9 — a per-lane walk runs at 28 % lane efficiency.  Instead every lane
// announces its count, an owner table in LDS maps item -> lane (wave-local, no barrier), and the wave works its ~250 items
// off 64 at a time, each lane fetching its item's Gaussian with ds_bpermute.  One item = one aligned tile pair of one rect
// row = (at most) one 64-bit atomic on the pair's counter word.
// ---------------------------------------------------------------------------------
// Pairs are aligned on the LINEAR tile index t = y * grid_x + x: a row of w tiles starting on an even t holds ceil(w / 2) of
// them, on an odd t floor(w / 2) + 1; on grids of odd width the rows of a rect alternate between the two.
struct RowPairs {
    int pa, pb;  // pairs in the rect's rows 0, 2, 4 ... and in its rows 1, 3, 5 ...
    __device__ __forceinline__ int per_two_rows() const { return pa + pb; }
    __device__ __forceinline__ int in_rows(int h) const { return ((h + 1) >> 1) * pa + (h >> 1) * pb; }
};
// t0: linear index of the rect's first tile, w: its width in tiles
__device__ __forceinline__ RowPairs row_pairs(int t0, int w, int grid_x) {
    const int t0b = t0 + grid_x;
    return {((t0 + w - 1) >> 1) - (t0 >> 1) + 1, ((t0b + w - 1) >> 1) - (t0b >> 1) + 1};
}
// multiplier of the small division q / ppr = (q * mul) >> 8 (q < 16, ppr <= 16: exact); 0 for a lane without items
__device__ __forceinline__ uint32_t pair_div_mul(int ppr) { return ppr > 0 ? (256u + (uint32_t)ppr - 1u) / (uint32_t)ppr : 0u; }

// "Announce": lane `lane` owns `cnt` items.  Scan the counts over the wave, fill the wave's owner table (item -> lane) and make
// it visible to the wave.  Returns the index of this lane's first item; ftotal = the wave's item count.
__device__ __forceinline__ uint32_t announce_items(uint8_t* own /* the wave's table */, int cnt, int lane, uint32_t& ftotal) {
    const uint32_t x = gsr::wave_inclusive_scan((uint32_t)cnt, lane);
    const uint32_t fpre = x - (uint32_t)cnt;
    ftotal = __shfl(x, 63);
    for (int k = 0; k < cnt; k++) own[fpre + k] = (uint8_t)lane;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return fpre;
}

// One decoded item.  The owner lane packs its rect as rlo = x0 | y0 << 16 and rhi = x1 | pair_div_mul(pairs per two rows) << 16
// (BANDED: y0 = the first row inside the band, and bits 26..31 of rhi = the mask bit of the clipped rect's first tile,
// (y0 - rect's y0) * w <= 32).
struct FlatItem {
    int src;            // owner lane
    uint32_t t;         // the pair's even tile (linear index; may lie left of the rect)
    int xe, y;          // ... and its tile coordinates
    bool va, vb;        // the even / odd tile belongs to the rect (both false on a lane past the last item)
    uint32_t kka, kkb;  // their bits in the emitted mask (row-major tile index inside the FULL rect, mod 32)
};
// item number `itu` of the wave's ftotal (> 0) items; every lane of the wave runs every trip — a ds_bpermute reads zero from
// a lane that is switched off
template <bool BANDED>
__device__ __forceinline__ FlatItem flat_item(const uint8_t* own, uint32_t itu, uint32_t ftotal, uint32_t fpre, uint32_t rlo,
                                              uint32_t rhi, int grid_x) {
    FlatItem f;
    const bool on = itu < ftotal;
    const uint32_t it = on ? itu : ftotal - 1u;
    f.src = own[it];
    const uint32_t q = it - __shfl(fpre, f.src);
    const uint32_t lo = __shfl(rlo, f.src), hi = __shfl(rhi, f.src), skb = BANDED ? hi >> 26 : 0u;
    const int x0 = (int)(lo & 0xFFFFu), y0 = (int)(lo >> 16), x1 = (int)(hi & 0xFFFFu);
    const int w = x1 - x0, t0 = y0 * grid_x + x0;
    const RowPairs rp = row_pairs(t0, w, grid_x);
    const int r2 = (int)((q * (BANDED ? (hi >> 16) & 0x3FFu : hi >> 16)) >> 8), rem = (int)q - r2 * rp.per_two_rows();  // (q < 16: exact)
    const int row = 2 * r2 + (rem >= rp.pa ? 1 : 0), pc = rem - (rem >= rp.pa ? rp.pa : 0);
    f.y = y0 + row;
    const int te = (((t0 + row * grid_x) >> 1) + pc) << 1;
    f.xe = te - f.y * grid_x;
    f.t = (uint32_t)te;
    f.va = on && f.xe >= x0;
    f.vb = on && f.xe + 1 < x1;
    f.kka = (skb + (uint32_t)(row * w + (f.xe - x0))) & 31u;
    f.kkb = (skb + (uint32_t)(row * w + (f.xe + 1 - x0))) & 31u;
    return f;
}

// The footprint tests of an item's two tiles on the owner's (broadcast) floats: exact-cull mode — a tile none of whose pixels
// can reach alpha >= 1/255 gets no instance (the reference keeps it and skips it pixel by pixel, render.jl:95).
__device__ __forceinline__ void item_may_touch(const GsrCam& cam, const FlatItem& f, const float m2[2], const float conic[3],
                                               float tau, uint32_t& c0, uint32_t& c1) {
    const float smx = __shfl(m2[0], f.src), smy = __shfl(m2[1], f.src);
    const float sa = __shfl(conic[0], f.src), sb = __shfl(conic[1], f.src), sc = __shfl(conic[2], f.src);
    const float stau = __shfl(tau, f.src);
    c0 = 0u; c1 = 0u;
    if (f.va) c0 = (!cam.exact_cull || tile_may_touch(smx, smy, sa, sb, sc, stau, f.xe * GSR_TILE, f.y * GSR_TILE)) ? 1u : 0u;
    if (f.vb) c1 = (!cam.exact_cull || tile_may_touch(smx, smy, sa, sb, sc, stau, (f.xe + 1) * GSR_TILE, f.y * GSR_TILE)) ? 1u : 0u;
}

// AGG: per counter word (an aligned tile pair), this workgroup's two counts, then its two bin positions — 2 x 32 bits, or
// 2 x 16 bits (W32) where a larger grid would not fit otherwise: a workgroup adds at most NT per tile, and a position that
// does not fit 16 bits is beyond bin_cap (the launcher checks) and is clamped to "not stored"
template <bool W32> using AggWord = typename std::conditional<W32, uint32_t, unsigned long long>::type;
template <bool W32>
__device__ __forceinline__ AggWord<W32> agg_inc(uint32_t c0, uint32_t c1) {
    return W32 ? (AggWord<W32>)(c0 | (c1 << 16)) : (AggWord<W32>)((unsigned long long)c0 | ((unsigned long long)c1 << 32));
}
template <bool W32>
__device__ __forceinline__ uint32_t agg_lo(AggWord<W32> v) { return W32 ? (uint32_t)v & 0xFFFFu : (uint32_t)v; }
template <bool W32>
__device__ __forceinline__ uint32_t agg_hi(AggWord<W32> v) {
    return W32 ? (uint32_t)v >> 16 : (uint32_t)((unsigned long long)v >> 32);
}
// an item's two instances as the emitted mask has them (SCATTER's restricted pass, only_above != 0: a tile whose list fits
// its bin takes no position here)
template <bool SCATTER>
__device__ __forceinline__ void replay(const FlatItem& f, const uint32_t* emit, uint32_t only_above,
                                       const uint32_t* __restrict__ tile_start, uint32_t& c0, uint32_t& c1) {
    const uint32_t em = emit[f.src];
    c0 = f.va ? (em >> f.kka) & 1u : 0u; c1 = f.vb ? (em >> f.kkb) & 1u : 0u;
    if (SCATTER && only_above) {
        if (c0) c0 = tile_start[f.t + 1u] - tile_start[f.t] > only_above ? 1u : 0u;
        if (c1) c1 = tile_start[f.t + 2u] - tile_start[f.t + 1u] > only_above ? 1u : 0u;
    }
}

// ---------------------------------------------------------------------------------
// The stages of preprocess_kernel (below) that are functions, each of the kernel's own per-lane state as separate arguments
// (as one struct the state moves the spill of the BANDED instantiations: profiles/pergauss_stages/codegen_compare.txt).
// ---------------------------------------------------------------------------------
constexpr int FLAT_MAX = 16;  // pair requests per lane up to which a rect takes the flattened walks

// SCATTER — the second pass of the compact mode: everything the walks need is in the record preprocess wrote.
//   in: the record of a Gaussian with radius > 0.  out: its state as project left it (no rgb / clamp bits: this pass neither
//   has nor needs them); `emitted` = the record's mask.
__device__ __forceinline__ void splat_from_record(const GsrGeoRec& rec, bool& visible, float m2[2], float conic[3], float& opac_v,
                                                  float& mc_z, int rmin[2], int rmax[2], uint32_t& area, float& tau, uint32_t& emitted) {
    visible = true;
    m2[0] = rec.q0.x; m2[1] = rec.q0.y; conic[0] = rec.q0.z; conic[1] = rec.q0.w; conic[2] = rec.q1.x;
    opac_v = rec.q1.y; mc_z = rec.q2.z;
    const uint32_t lo = __float_as_uint(rec.q3.x), hi = __float_as_uint(rec.q3.y);
    rmin[0] = (int)(lo & 0xFFFFu); rmin[1] = (int)(lo >> 16); rmax[0] = (int)(hi & 0xFFFFu); rmax[1] = (int)(hi >> 16);
    area = (uint32_t)((rmax[0] - rmin[0]) * (rmax[1] - rmin[1]));
    tau = footprint_tau(opac_v);
    emitted = __float_as_uint(rec.q3.w);
}

// The DIRECT form of the flattened walk: an item = one pair request = (at most) one returning global atomic; two rounds of
// items in flight per lane.
//   in: the rect, the footprint floats, the depth, this lane's walk class (fcnt, fppr); own / emit: this wave's owner table and
//   mask row in LDS.  out: tile_count and bins; `emitted` of the lanes that took the walk (fcnt > 0).  No template flag but NT.
template <int NT>
__device__ __forceinline__ void emit_direct(const GsrCam& cam, int fcnt, int fppr, const float m2[2], const float conic[3], float tau,
                                            float mc_z, const int rmin[2], const int rmax[2], uint8_t* own, uint32_t* emit,
                                            uint32_t* __restrict__ tile_count, uint64_t* __restrict__ bins, uint32_t bin_cap,
                                            uint32_t& emitted) {
    const int ln = threadIdx.x & 63;
    unsigned long long* tc64 = reinterpret_cast<unsigned long long*>(tile_count);
    emit[ln] = 0u;
    uint32_t ftotal;
    const uint32_t fpre = announce_items(own, fcnt, ln, ftotal);
    const uint32_t rlo = (uint32_t)rmin[0] | ((uint32_t)rmin[1] << 16);
    const uint32_t rhi = (uint32_t)rmax[0] | (pair_div_mul(fppr) << 16);
    constexpr int INFL = 2;
    for (uint32_t base = 0; base < ftotal; base += 64u * INFL) {
        uint32_t tt[INFL], cc[INFL], zz[INFL], ss[INFL];
        unsigned long long old[INFL];
#pragma unroll
        for (int u = 0; u < INFL; u++) {
            const FlatItem f = flat_item<false>(own, base + 64u * (uint32_t)u + (uint32_t)ln, ftotal, fpre, rlo, rhi, cam.grid_x);
            zz[u] = __shfl(__float_as_uint(mc_z), f.src);
            ss[u] = (uint32_t)f.src;
            tt[u] = f.t;
            uint32_t c0, c1;
            item_may_touch(cam, f, m2, conic, tau, c0, c1);
            cc[u] = c0 | (c1 << 1);
            if (cc[u]) {
                atomicOr(&emit[f.src], (c0 << f.kka) | (c1 << f.kkb));
                old[u] = atomicAdd(tc64 + (tt[u] >> 1), (unsigned long long)c0 | ((unsigned long long)c1 << 32));
            }
        }
#pragma unroll
        for (int u = 0; u < INFL; u++)
            if (cc[u]) {
                const uint64_t skey = ((uint64_t)zz[u] << 32) | (uint32_t)(blockIdx.x * NT + (threadIdx.x & ~63) + ss[u]);
                const uint32_t p0 = (uint32_t)old[u], p1 = (uint32_t)(old[u] >> 32);
                if ((cc[u] & 1u) && p0 < bin_cap) bins[(size_t)tt[u] * bin_cap + p0] = skey;
                if ((cc[u] & 2u) && p1 < bin_cap) bins[(size_t)(tt[u] + 1) * bin_cap + p1] = skey;
            }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (fcnt > 0) emitted = emit[ln];
}

// Large footprints: one thread walking hundreds of tiles serialises the wave (the reference's
// duplicate_with_keys! has exactly this loop, utils.jl:96-119).  Rects of more than EMIT_COOP
// tiles are emitted by the whole wave, one tile per lane and round — same tests on the same
// (broadcast) floats, so the lists are identical.
//   in: the rect (rmin, rmax, area), the footprint floats (m2, conic, tau), the depth; coop_small: a rect of at most EMIT_COOP
//   tiles with more than FLAT_MAX pair requests joins.  out: tile_count and bins (SCATTER: the fill counters and the compact
//   keys at tile_start, restricted by only_above); !SCATTER: `emitted` of a joined rect of at most DENSE_RECT tiles.
//   Depends on NT (the key) and SCATTER.
template <int NT, bool SCATTER>
__device__ __forceinline__ void emit_cooperative(const GsrCam& cam, bool visible, uint32_t area, bool coop_small, const float m2[2],
                                                 const float conic[3], float tau, const int rmin[2], const int rmax[2], float mc_z,
                                                 uint32_t only_above, uint32_t bin_cap, const uint32_t* __restrict__ tile_start,
                                                 uint32_t* __restrict__ tile_count, uint64_t* __restrict__ bins, uint32_t& emitted) {
    const int lane = threadIdx.x & 63;
    unsigned long long big = __builtin_amdgcn_ballot_w64(visible && (area > EMIT_COOP || coop_small));
    while (big) {
        const int src = __builtin_ctzll(big);
        big &= big - 1;
        const float bmx = __shfl(m2[0], src), bmy = __shfl(m2[1], src);
        const float ba = __shfl(conic[0], src), bb = __shfl(conic[1], src), bc = __shfl(conic[2], src);
        const float btau = __shfl(tau, src);
        const int bx0 = __shfl(rmin[0], src), by0 = __shfl(rmin[1], src);
        const int bx1 = __shfl(rmax[0], src), by1 = __shfl(rmax[1], src);
        const uint32_t bz = __shfl(__float_as_uint(mc_z), src);
        const uint64_t bkey = ((uint64_t)bz << 32) | (uint32_t)(blockIdx.x * NT + (threadIdx.x & ~63) + src);
        const int w = bx1 - bx0, total = w * (by1 - by0);
        uint32_t first32 = 0u;  // which of the rect's first 32 tiles got an instance (its emitted mask when it is a small one)
        for (int e = lane; e < total; e += 64) {
            const int ry = e / w, rx = e - ry * w;
            const int x = bx0 + rx, y = by0 + ry;
            const bool pass = !cam.exact_cull || tile_may_touch(bmx, bmy, ba, bb, bc, btau, x * GSR_TILE, y * GSR_TILE);
            if (e < 64) first32 = (uint32_t)__builtin_amdgcn_ballot_w64(pass);  // (lane 0 is in the first trip)
            if (pass) {
                const uint32_t t = (uint32_t)(y * cam.grid_x + x);
                if (SCATTER) {
                    const uint32_t ts = tile_start[t];
                    if (!only_above || tile_start[t + 1u] - ts > only_above) bins[ts + atomicAdd(tile_count + t, 1u)] = bkey;
                } else {
                    const uint32_t pos = atomicAdd(tile_count + t, 1u);
                    if (pos < bin_cap) bins[(size_t)t * bin_cap + pos] = bkey;
                }
            }
        }
        first32 = __shfl(first32, 0);
        if (!SCATTER && lane == src && (uint32_t)total <= DENSE_RECT) emitted = first32;
    }
}

// ---------------------------------------------------------------------------------
// preprocess: project! (projection.jl:69-129) + spherical_harmonics!
// (spherical_harmonics.jl:12-17,41-74) + count_tiles_per_gaussian! (utils.jl:131-141),
// and the per-tile occupancy histogram that replaces cumsum!/duplicate/sort-by-tile.
// ---------------------------------------------------------------------------------
//   Two forms of the binning.  DIRECT (AGG_NT == 0): one returning global atomic per instance pair, as described below.
// AGGREGATING (large scenes on grids whose counter words fit the LDS three times per CU): what the global atomics cost on
// this part is the number of memory transactions a wave instruction makes (tools/atomic_rates.hip: 64 lanes on 64 random
// counter words run at 24 G atomics/s, on 64 consecutive words at 130 G/s), and one Gaussian per lane in the scene's
// order means 64 random words per instruction.  A workgroup of AGG_NT Gaussians therefore (1) adds its requests up per
// counter word in LDS (one 64-bit word per aligned tile pair, the global counters' packing), (2) issues ONE returning
// global atomic per word it counted in — consecutive lanes on consecutive words; the LDS word then holds the bin
// positions this workgroup's instances start at (config 3, 512 Gaussians: ~1 500 requests on ~1 250 of the 4 081 words,
// 16 % fewer global atomics, in address order), (3) re-walks its rects, the footprint tests replayed from the emitted
// mask, every instance taking its position with a returning LDS atomic, and stores the keys.  Both walks are flattened
// over the lanes of each wave (below: 28 % -> ~95 % lane efficiency).  Three workgroups per CU in
// several rounds, so that the phases of different workgroups overlap (1024 Gaussians per workgroup aggregate better and
// were measured slower: 0.19 ms against 0.15; so was one resident wave of persistent workgroups).  The order inside a
// bin differs from the direct form's (it is arbitrary in both; the tile sort fixes it); everything else is bit-identical.
//   n_words: 64-bit words of the counter array = LDS words of the AGG form ((T + 2) / 2).
template <int DEG, int AGG_NT /* 0: direct form, 256 threads; else the threads of the aggregating workgroup */,
          bool W32 = false /* aggregating form with 2 x 16-bit LDS words (grids whose 64-bit words do not fit; positions < 65 024) */,
          bool SCATTER = false /* the compact binning mode's SECOND pass (duplicate_with_keys! as count -> scan -> scatter): no
                                  projection — the geometry records are read back —, keys go to tile_start[t] + arrival rank */,
          bool BANDED = false /* aggregating form over horizontal bands of the tile grid (n_bands > 1); false: ONE band = the whole
                                 grid, the band loop and the rect clipping compile away (round 4's kernel, register for register) */,
          bool AA = false /* antialiased handle (GSR_FLAG_ANTIALIASED): the opacity every later stage sees is the caller's times the
                             compensation of add_blur, which goes to `comp`; a template flag, so that the default kernels are the
                             parent's register for register (the aggregating forms sit ON their occupancy step) */>
// (direct form: AT MOST four waves per SIMD — with its per-lane walks gone it would fit five, and five waves of scattered returning
//  atomics are slower than four: config 5 0.66-0.68 ms against 0.60-0.62)
__global__ __launch_bounds__(AGG_NT ? AGG_NT : 256)
__attribute__((amdgpu_waves_per_eu(AGG_NT ? 3 * AGG_NT / 256 : 1, AGG_NT ? 8 : 4))) void preprocess_kernel(int n, int K, int channels,
                                                                      const float* __restrict__ means,
                                                                      const float* __restrict__ scales,
                                                                      const float4* __restrict__ rots,
                                                                      const float* __restrict__ opac,
                                                                      const float* __restrict__ shs, GsrCam cam,
                                                                      GsrGeom geom, uint32_t* __restrict__ tile_count,
                                                                      uint32_t* __restrict__ n_visible,
                                                                      uint64_t* __restrict__ bins, uint32_t bin_cap,
                                                                      int n_words, const uint32_t* __restrict__ tile_start,
                                                                      int n_bands, int band_rows,
                                                                      float* __restrict__ comp /* AA: compensations (N) */) {
    static_assert(!SCATTER || AGG_NT != 0, "the scatter pass exists in the aggregating form only");
    static_assert(!SCATTER || !AA, "the scatter pass replays the record: the effective opacity is in it");
    static_assert(!BANDED || AGG_NT != 0, "bands are the aggregating form's");
    constexpr bool AGG = AGG_NT != 0;
    constexpr int NT = AGG ? AGG_NT : 256;
    using Word = AggWord<W32>;
    extern __shared__ unsigned long long agg_raw[];
    Word* agg = reinterpret_cast<Word*>(agg_raw);
    const int i = blockIdx.x * NT + threadIdx.x;
    // SCATTER: `bin_cap` carries only_above — 0: every tile; else only the tiles whose list is longer (the lists that overflowed
    // the fixed-capacity bins: the others' keys sit complete in their bins, round 5)
    const uint32_t only_above = SCATTER ? bin_cap : 0u;
    (void)n_words; (void)only_above;
    bool visible = false;
    uint32_t area = 0, clamp_bits = 0, emitted = 0;  // emitted: bit k = tile k of the rect (row-major) got an instance
    float m2[2] = {0, 0}, conic[3] = {0, 0, 0}, rgb[3] = {0, 0, 0}, mc_z = 0.0f, tau = 0.0f, opac_v = 0.0f;
    int rmin[2] = {0, 0}, rmax[2] = {0, 0};
    // SH colour of Gaussian i at world position p (spherical_harmonics.jl:12-17,41-74)
    auto sh_colour = [&](const float p[3]) {
        const float* sh = shs + (size_t)3 * K * i;
        float d0[3], d[3];
        view_dir(p, cam.center, d0, d);
        float b[16];
        sh_basis<DEG>(d, b);
        constexpr int NB = (DEG + 1) * (DEG + 1);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float res = b[0] * sh[c];
#pragma unroll
            for (int k = 1; k < NB; k++) res = res + b[k] * sh[3 * k + c];
            res = res + 0.5f + 1.1920929e-7f;
            if (res < 0.0f) clamp_bits |= 1u << c;
            rgb[c] = fmaxf(0.0f, res);
        }
    };
    if (SCATTER) {
        if (i < n && geom.radii[i] > 0) {
            splat_from_record(geom.rec[i], visible, m2, conic, opac_v, mc_z, rmin, rmax, area, tau, emitted);
        }
    } else if (i < n) {
        M33 R; float t[3];
        load_pose(cam, R, t);
        // the small inputs of this Gaussian are requested up front (one round trip instead of three dependent ones:
        // means -> rotation/scale -> opacity); 14 % of them turn out culled and waste 28 bytes each
        const float p[3] = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
        const float4 q_in = rots[i];
        const float s_in[3] = {scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]};
        const float opac_in = opac[i];
        opac_v = opac_in;
        float mc[3];
#pragma unroll
        for (int r = 0; r < 3; r++) mc[r] = (R.m[r][0] * p[0] + R.m[r][1] * p[1] + R.m[r][2] * p[2]) + t[r];
        mc_z = mc[2];
        int radius = 0;
        float rho = 0.0f;  // AA: add_blur's compensation
        M33 Rg; float s[3];
        if (cam.near_plane < mc[2] && mc[2] < cam.far_plane) {
            float qn[4], inv_norm;
            Rg = quat2rot(q_in, qn, inv_norm);
            s[0] = s_in[0]; s[1] = s_in[1]; s[2] = s_in[2];
            M33 M;
            M33 Sigma = cov3d(Rg, s, M);
            M33 Sc = mul33(mul33(R, Sigma), tr33(R));
            Persp pr = persp_common(mc, cam);
            const int res[2] = {cam.width, cam.height};
#pragma unroll
            for (int k = 0; k < 2; k++) {
                float pp = cam.principal[k] * (float)res[k];
                m2[k] = pr.rz * cam.focal[k] * mc[k] + pp;
            }
            float JS[2][3];
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 3; b++)
                    JS[a][b] = pr.J[a][0] * Sc.m[0][b] + pr.J[a][1] * Sc.m[1][b] + pr.J[a][2] * Sc.m[2][b];
            M22 S2;
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++)
                    S2.m[a][b] = JS[a][0] * pr.J[b][0] + JS[a][1] * pr.J[b][1] + JS[a][2] * pr.J[b][2];
            // add_blur (render.jl:387-396)
            float det_orig = 0.0f;
            if constexpr (AA) det_orig = S2.m[0][0] * S2.m[1][1] - S2.m[0][1] * S2.m[1][0];
            S2.m[0][0] = S2.m[0][0] + cam.blur_eps;
            S2.m[1][1] = S2.m[1][1] + cam.blur_eps;
            float det = S2.m[0][0] * S2.m[1][1] - S2.m[0][1] * S2.m[1][0];
            if (det > 0.0f) {
                if constexpr (AA) rho = sqrtf(fmaxf(0.0f, det_orig / det));
                // inverse (render.jl:368-381)
                float det_inv = 1.0f / det;
                float tmp = -S2.m[0][1] * det_inv;
                conic[0] = S2.m[1][1] * det_inv; conic[1] = tmp; conic[2] = S2.m[0][0] * det_inv;
                // max_eigval_2D (render.jl:415-420)
                float mid = 0.5f * (S2.m[0][0] + S2.m[1][1]);
                float lam = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
                int rad = (int)ceilf(3.0f * sqrtf(lam));
                bool off = (m2[0] + (float)rad) <= 0.0f || (m2[0] - (float)rad) >= (float)res[0] ||
                           (m2[1] + (float)rad) <= 0.0f || (m2[1] - (float)rad) >= (float)res[1];
                if (rad > cam.radius_clip && !off) radius = rad;
            }
        }
        geom.radii[i] = radius;
        if (radius > 0) {
            visible = true;
            // (the normal first: it is the last reader of R, Rg, s and mc — 24 registers that would otherwise stay allocated
            //  across the SH stage, the kernel's register peak, whatever the render mode: 114 -> 100 VGPRs)
            if (channels > 5) {
                float nn[3]; int k; float sg;
                gaussian_normal(R, Rg, s, mc, nn, k, sg);
                geom.normal[i] = make_float4(nn[0], nn[1], nn[2], 0.0f);
            }
            sh_colour(p);
            get_rect(m2[0], m2[1], radius, cam.grid_x, cam.grid_y, rmin, rmax);
            area = (uint32_t)((rmax[0] - rmin[0]) * (rmax[1] - rmin[1]));
            if constexpr (AA) {
                // an antialiased render of opacities o IS the plain render of o * rho: every reader of the opacity below — the
                // footprint test, the record, the blend threshold — takes the product.  rho == 0 (a footprint whose fp32
                // det_orig is <= 0): tau = log(0) emits nothing.  comp[i] stays stale where radii == 0, like the record.
                comp[i] = rho;
                opac_v = opac_in * rho;
            }
            tau = footprint_tau(opac_v);
        }
    }
    // duplicate_with_keys! (utils.jl:85-120) restated per tile, fused into this kernel: the
    // instance takes the next free position of its tile's BIN (a fixed-capacity segment of
    // `bins`, capacity from the previous view) with a returning atomic on the tile's counter
    // and stores its (depth bits << 32 | id) key there — the counters end up holding the
    // reference's per-tile counts, and no separate count / scan / scatter pass over the
    // instances exists.  Horizontally adjacent tiles are consecutive 32-bit counters, so an
    // aligned pair is served by ONE 64-bit atomic; two rounds of them are kept in flight per
    // lane before their keys are stored (a returning device-scope atomic is a ~2 us round trip
    // to the memory side).  A position >= bin_cap is not stored: the host sees max count >
    // capacity in the scan's totals, grows the bins and repeats the pass (first view / a much
    // denser view).
    // Rects of at most EMIT_COOP tiles take the flattened walks (flat_item above); Gaussians of more than FLAT_MAX requests
    // (1 %) join the wave-cooperative path below, which then also leaves their emitted mask.
    __shared__ uint8_t own_tab[NT / 64][64 * FLAT_MAX];
    __shared__ uint32_t emit_tab[NT / 64][64];
    const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int rw_ = rmax[0] - rmin[0];
    int fcnt = 0, fppr = 0;          // this lane's pair requests in the flattened walks, pairs per TWO rows of its rect
    bool coop_small = false;         // ... or too many of them: with the wave-cooperative path
    if (visible && area <= EMIT_COOP) {
        const RowPairs rp = row_pairs(rmin[1] * cam.grid_x + rmin[0], rw_, cam.grid_x);
        fppr = rp.per_two_rows();
        fcnt = rp.in_rows(rmax[1] - rmin[1]);
        if (fcnt > FLAT_MAX) { fcnt = 0; coop_small = true; }
    }
    unsigned long long* tc64 = reinterpret_cast<unsigned long long*>(tile_count);
    if (!AGG) {
        emit_direct<NT>(cam, fcnt, fppr, m2, conic, tau, mc_z, rmin, rmax, own_tab[wv], emit_tab[wv], tile_count, bins, bin_cap, emitted);
    } else {
        // AGGREGATING form, in horizontal BANDS of the tile grid (round 5: n_bands == 1 is round 4's kernel).  The counter words of
        // a 4K grid do not fit the LDS three times per CU; the words of HALF the grid do — so the workgroup runs its two walks
        // once per band of `band_rows` tile rows, every rect clipped to the band: the same items, the same tests, the same
        // positions (a rect's rows are walked band by band instead of in one go; the emitted mask is indexed by the row inside the
        // FULL rect).  What the LDS buys on a large grid is not fewer global atomics (a 512-Gaussian workgroup hits mostly distinct
        // words there) but (a) their address order and (b) no same-address serialisation: a hot tile's instances meet in LDS first
        // (dense scenes: 1 % of a 4K grid at 50 x density took the direct form 1.9 ms).
        // (This stage, the projection above, sh_colour and the slot scan below stay in the kernel's body: as functions they cost
        //  scalar loads, VGPRs, spill or time in some instantiation — profiles/pergauss_stages/codegen_compare.txt.)
        const bool flat_lane = fcnt > 0;  // this lane's rect takes the flattened walks
        emit_tab[wv][ln] = SCATTER ? emitted : 0u;  // SCATTER replays the record's mask; else the first walk's tests fill it
        for (int band = 0; band < (BANDED ? n_bands : 1); band++) {
            const int yb0 = BANDED ? band * band_rows : 0, yb1 = BANDED ? min(cam.grid_y, yb0 + band_rows) : cam.grid_y;
            const int wbase = BANDED ? (yb0 * cam.grid_x) >> 1 : 0;
            const int wcount = BANDED ? ((yb1 * cam.grid_x - 1) >> 1) - wbase + 1 : n_words;
            if (BANDED && band > 0) __syncthreads();  // the previous band's second walk has taken its positions
            for (int w = threadIdx.x; w < wcount; w += NT) agg[w] = (Word)0;
            // this lane's rect clipped to the band
            const int yc0 = BANDED ? max(rmin[1], yb0) : rmin[1], yc1 = BANDED ? min(rmax[1], yb1) : rmax[1];
            int bcnt = BANDED ? 0 : fcnt, bppr = BANDED ? 0 : fppr;
            if (BANDED && flat_lane && yc1 > yc0) {
                const RowPairs rp = row_pairs(yc0 * cam.grid_x + rmin[0], rw_, cam.grid_x);
                bppr = rp.per_two_rows();
                bcnt = rp.in_rows(yc1 - yc0);
            }
            uint32_t ftotal;
            const uint32_t fpre = announce_items(own_tab[wv], bcnt, ln, ftotal);
            const uint32_t rlo = (uint32_t)rmin[0] | ((uint32_t)yc0 << 16);
            const uint32_t rhi = (uint32_t)rmax[0] | (pair_div_mul(bppr) << 16) |
                                 (BANDED ? (uint32_t)((yc0 - rmin[1]) * rw_) << 26 : 0u);
            __syncthreads();  // agg zeroed
            // first walk: count per word
            for (uint32_t base = 0; base < ftotal; base += 64u) {
                const FlatItem f = flat_item<BANDED>(own_tab[wv], base + (uint32_t)ln, ftotal, fpre, rlo, rhi, cam.grid_x);
                uint32_t c0, c1;
                if (SCATTER) replay<SCATTER>(f, emit_tab[wv], only_above, tile_start, c0, c1);
                else item_may_touch(cam, f, m2, conic, tau, c0, c1);
                if (c0 | c1) {
                    if (!SCATTER) atomicOr(&emit_tab[wv][f.src], (c0 << f.kka) | (c1 << f.kkb));
                    atomicAdd(&agg[(f.t >> 1) - (uint32_t)wbase], agg_inc<W32>(c0, c1));
                }
            }
            __syncthreads();
            // one global atomic per word this workgroup counted in; the word then holds the positions its instances start at
            for (int w0 = threadIdx.x; w0 < wcount; w0 += 4 * NT) {  // four in flight per lane
                unsigned long long old[4];
                uint32_t any = 0u;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const Word c = w0 + k * NT < wcount ? agg[w0 + k * NT] : (Word)0;
                    if (c) {
                        old[k] = atomicAdd(tc64 + wbase + w0 + k * NT,
                                           (unsigned long long)agg_lo<W32>(c) | ((unsigned long long)agg_hi<W32>(c) << 32));
                        any |= 1u << k;
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (any & (1u << k)) {
                        if (W32) {
                            const uint32_t lim = 0xFFFFu - (uint32_t)NT;  // (beyond every stored position: "not stored", and no carry into the other half)
                            agg[w0 + k * NT] = (Word)(min((uint32_t)old[k], lim) | (min((uint32_t)(old[k] >> 32), lim) << 16));
                        } else {
                            agg[w0 + k * NT] = (Word)old[k];
                        }
                    }
            }
            __syncthreads();
            if (SCATTER || bin_cap > 0u) {
                // second walk: the same items, the tests replayed from the emitted mask, every instance takes its position
                for (uint32_t base = 0; base < ftotal; base += 64u) {
                    const FlatItem f = flat_item<BANDED>(own_tab[wv], base + (uint32_t)ln, ftotal, fpre, rlo, rhi, cam.grid_x);
                    const uint32_t zb = __shfl(__float_as_uint(mc_z), f.src);
                    uint32_t c0, c1;
                    replay<SCATTER>(f, emit_tab[wv], only_above, tile_start, c0, c1);
                    if (c0 | c1) {
                        const Word old = atomicAdd(&agg[(f.t >> 1) - (uint32_t)wbase], agg_inc<W32>(c0, c1));
                        const uint64_t skey = ((uint64_t)zb << 32) | (uint32_t)(blockIdx.x * NT + (threadIdx.x & ~63) + f.src);
                        const uint32_t p0 = agg_lo<W32>(old), p1 = agg_hi<W32>(old);
                        if (SCATTER) {
                            if (c0) bins[tile_start[f.t] + p0] = skey;
                            if (c1) bins[tile_start[f.t + 1u] + p1] = skey;
                        } else {
                            if (c0 && p0 < bin_cap) bins[(size_t)f.t * bin_cap + p0] = skey;
                            if (c1 && p1 < bin_cap) bins[(size_t)(f.t + 1) * bin_cap + p1] = skey;
                        }
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (!SCATTER && flat_lane) emitted = emit_tab[wv][ln];
    }
    emit_cooperative<NT, SCATTER>(cam, visible, area, coop_small, m2, conic, tau, rmin, rmax, mc_z, only_above, bin_cap, tile_start,
                                  tile_count, bins, emitted);
    // Exclusive scan of the tile-rect areas inside the block: with bpre[block] (tile_scan) it
    // gives every Gaussian the offset of its instance slots (gradient rows) — the reference's
    // cumsum!(tiles_touched) (rasterizer.jl:333-335), restated hierarchically.
    if (!SCATTER) {
        // (blocks of 256 Gaussians whatever the workgroup size: bpre[i >> 8] is what the readers index)
        __shared__ uint32_t wsum[NT / 64];
        __shared__ uint32_t wvis[NT / 64];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wave0 = wave & ~3;
        // gradient-row slots of this Gaussian: one per emitted tile (small rects), one per tile of the rect otherwise
        const uint32_t slots = area <= DENSE_RECT ? (uint32_t)__popc(emitted) : area;
        const uint32_t x = gsr::wave_inclusive_scan(slots, lane);
        const unsigned long long vm = __ballot(visible);
        // (high half: the visible Gaussians whose rect holds at least one tile — the reference's instance count is > 0 iff any)
        const unsigned long long am = __ballot(visible && area > 0u);
        if (lane == 63) { wsum[wave] = x; wvis[wave] = (uint32_t)__popcll(vm) | ((uint32_t)__popcll(am) << 16); }
        __syncthreads();
        uint32_t woff = 0;
        for (int w = wave0; w < wave; w++) woff += wsum[w];
        const uint32_t lpre = woff + x - slots;
        if ((threadIdx.x & 255) == 255 && i - 255 < n) {
            geom.bsum[i >> 8] = lpre + slots;
            // visible count per block, summed by tile_scan (15 k same-address atomics would
            // serialise at ~12 ns each: 0.19 ms — the "fanin" price of MI355X_MICROARCH.md)
            n_visible[i >> 8] = wvis[wave0] + wvis[wave0 + 1] + wvis[wave0 + 2] + wvis[wave0 + 3];
        }
        if (visible) {
            GsrGeoRec rec;
            rec.q0 = make_float4(m2[0], m2[1], conic[0], conic[1]);
            rec.q1 = make_float4(conic[2], opac_v, rgb[0], rgb[1]);
            rec.q2 = make_float4(rgb[2], __uint_as_float(clamp_bits), mc_z, __uint_as_float(lpre));
            rec.q3 = make_float4(__uint_as_float((uint32_t)rmin[0] | ((uint32_t)rmin[1] << 16)),
                                 __uint_as_float((uint32_t)rmax[0] | ((uint32_t)rmax[1] << 16)),
                                 __uint_as_float(blend_threshold_bits(opac_v)), __uint_as_float(emitted));
            geom.rec[i] = rec;
        }
    }
}

}  // namespace

// The aggregating form's LDS plan (agg_plan.h): whole grid or bands, 2 x 32-bit or 2 x 16-bit words.
namespace {
using AggPlan = gsr_agg::Plan;
inline AggPlan agg_plan(int grid_x, int grid_y, uint32_t max_pos) { return gsr_agg::plan(grid_x, grid_y, max_pos); }
using gsr::dispatch_bool;
using gsr::dispatch_degree;
}  // namespace

// `agg`: the aggregating form (else the direct one) — WHICH is gsr_policy.cpp's decision (gsr_policy_begin_view: the handle's
// pin, the process default, the scene / grid rule with the previous view's skew, or the form tuner's measurement).  Returns
// the form that ran (gsr_stats.preprocess_form = gsr_agg::form_code: the same number the policy announced).
int gsr_launch_preprocess(hipStream_t s, int n, int K, int degree, int channels, const float* means,
                          const float* scales, const float* rots, const float* opac, const float* shs, GsrCam cam,
                          GsrGeom geom, GsrTiles tiles, uint32_t* n_visible, GsrKeys keys, bool agg, float* comp) {
    if (n <= 0) return 0;
    const float4* r4 = reinterpret_cast<const float4*>(rots);
    // The aggregating form keeps its counter words in LDS three times per CU: the whole grid up to ~21 500 tiles, bands of it
    // beyond (4K: two).
    const int n_words = (tiles.n_tiles + 2) / 2;
    const AggPlan pl = agg_plan(cam.grid_x, cam.grid_y, keys.cap);
    const uint32_t* no_start = nullptr;
    dispatch_degree(degree, [&](auto d) {
        constexpr int DEG = d;
        dispatch_bool(comp != nullptr, [&](auto a) {
            constexpr bool AA = a;
            if (!agg) {
                hipLaunchKernelGGL((preprocess_kernel<DEG, 0, false, false, false, AA>), dim3((n + 255) / 256), dim3(256), 0, s, n,
                                   K, channels, means, scales, r4, opac, shs, cam, geom, tiles.count, n_visible, keys.bins,
                                   keys.cap, n_words, no_start, 1, cam.grid_y, comp);
                return;
            }
            dispatch_bool(pl.w32, [&](auto w) {
                constexpr bool W32 = w;
                dispatch_bool(pl.n_bands > 1, [&](auto b) {
                    constexpr bool BANDED = b;
                    hipLaunchKernelGGL((preprocess_kernel<DEG, kAggThreads, W32, false, BANDED, AA>),
                                       dim3((n + kAggThreads - 1) / kAggThreads), dim3(kAggThreads), pl.lds, s, n, K, channels,
                                       means, scales, r4, opac, shs, cam, geom, tiles.count, n_visible, keys.bins, keys.cap,
                                       n_words, no_start, pl.n_bands, pl.band_rows, comp);
                });
            });
        });
    });
    return gsr_agg::form_code(agg, pl);
}

// duplicate_with_keys! (utils.jl:85-120) as the SECOND pass of the compact binning mode (count -> scan -> scatter): the
// aggregating form of preprocess_kernel in its SCATTER instantiation — the records are read back, the walks replay the emitted
// masks, the positions handed out are arrival ranks inside tile_start[t] ... — so that a hot tile's instances meet in LDS
// instead of serialising on one global counter (round 4's per-lane kernel: 0.85 ms for one tile of 32 k instances, 2.4 ms
// on a 4K grid with 1 % of the tiles at 50 x density).  `max_list`: the longest tile list (the scan's total), which decides
// between 2 x 16-bit and 2 x 32-bit LDS words.
void gsr_launch_emit_compact(hipStream_t s, int n, GsrCam cam, GsrGeom geom, const uint32_t* tile_start, uint32_t* tile_fill,
                             uint64_t* keys, uint32_t max_list, uint32_t only_above) {
    if (n <= 0) return;
    const AggPlan pl = agg_plan(cam.grid_x, cam.grid_y, max_list);
    const int n_words = (cam.grid_x * cam.grid_y + 2) / 2;
    const dim3 grid((n + kAggThreads - 1) / kAggThreads), block(kAggThreads);
    const float* nf = nullptr;
    const float4* nq = nullptr;
    dispatch_bool(pl.w32, [&](auto w) {
        constexpr bool W32 = w;
        dispatch_bool(pl.n_bands > 1, [&](auto b) {
            constexpr bool BANDED = b;
            hipLaunchKernelGGL((preprocess_kernel<0, kAggThreads, W32, true, BANDED>), grid, block, pl.lds, s, n, 0, 3, nf,
                               nf, nq, nf, nf, cam, geom, tile_fill, (uint32_t*)nullptr, keys, only_above, n_words, tile_start,
                               pl.n_bands, pl.band_rows, (float*)nullptr);
        });
    });
}
