// mgp_zs.hip — the fused smoothing phases' host side: the tile settings read from the environment, tile and z-chunk
// planning, k_zs's fp32 instantiations (launcher, dispatch and attributes: mgp_zs.h; fp64: mgp_zs_f64.hip),
// prepare_kernels and launch_fused.
#include "mgp_zs.h"

#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>

namespace mgp {

// ---- fused smoothing phases ----

static int parse_patch(const char* v, int dflt)
{
    int px = 0, py = 0;
    if (!v) return dflt;
    if (std::sscanf(v, "%d,%d", &px, &py) != 2 || px < 1 || py < 1 || px > 255 || py > 255) return 0;
    return px | (py << 8);
}

FusedTuning fused_tuning_from_env()
{
    FusedTuning t;
    if (const char* v = std::getenv("MGP_ZS_WIDE")) t.wide = std::atoi(v) != 0;
    if (const char* v = std::getenv("MGP_YS_HALF")) t.ys_half = std::atoi(v);
    if (const char* v = std::getenv("MGP_YS_ROWS")) {
        const int r = std::atoi(v);
        t.ys_rows = r >= 8 && (r & 1) == 0 ? r : 32;
    }
    if (const char* v = std::getenv("MGP_ZS_WGS")) t.wgs = std::max<int64_t>(1, std::atoll(v));
    const char* vb = std::getenv("MGP_ZS_PATCH");
    const int both = parse_patch(vb, 0);
    t.patch_pre = parse_patch(std::getenv("MGP_ZS_PATCH_PRE"), both);
    // POST's default: 4 x 8 patches on planes of >= 4096 tiles (auto, -1; round 5: the configs[4] slab's POST
    // 32.7 -> 30.8 ms per F-cycle, while on the configs[3] slab's 2048 tiles per plane it lost 3.50 -> 3.80 ms)
    t.patch_post = parse_patch(std::getenv("MGP_ZS_PATCH_POST"), vb ? both : -1);
    if (const char* v = std::getenv("MGP_ZS_FWF")) t.fwf = std::atoi(v) != 0;
    if (const char* v = std::getenv("MGP_ZS_POST_ZC")) t.post_zc = std::max(0, std::atoi(v));
    if (const char* v = std::getenv("MGP_ZS_SPLIT")) t.split = std::atoi(v) != 0;
    if (const char* v = std::getenv("MGP_ZS_SPLIT_CL")) t.split_cl = std::atoi(v) != 0;
    if (const char* v = std::getenv("MGP_ZPOST_PRE")) t.zpost_pre = std::atoi(v) != 0;
    if (const char* v = std::getenv("MGP_ZS_SPLIT_POST")) t.split_post = std::atoi(v) != 0;
    if (const char* v = std::getenv("MGP_ZS_SPLIT_POST_MIN_CELLS")) t.split_post_min_cells = std::max<int64_t>(0, std::atoll(v));
    if (const char* v = std::getenv("MGP_STAMP_R")) t.stamp_r = std::atoi(v) != 0;
    return t;
}

// tile of a phase (pre) or the largest of all (pre < 0); clz: the level operator has no boundary modification;
// wide: POST's wide tile (zs_wide)
static void zs_tile(int rb, int& tx, int& ty, int pre = -1, bool clz = true, bool wide = false)
{
    const int xa = rb == 4 ? ZsTile<float>::TXPRE : ZsTile<double>::TXPRE;
    const int xc = rb == 4 ? ZsTile<float>::TXPRE_CL : ZsTile<double>::TXPRE_CL;
    const int xb = rb == 4 ? ZsTile<float>::TXPOST : ZsTile<double>::TXPOST;
    const int a = rb == 4 ? ZsTile<float>::TYPRE : ZsTile<double>::TYPRE;
    const int ac = rb == 4 ? ZsTile<float>::TYPRE_CL : ZsTile<double>::TYPRE_CL;
    const int b = rb == 4 ? ZsTile<float>::TYPOST : ZsTile<double>::TYPOST;
    const int xp = clz ? xa : xc, yp = clz ? a : ac;
    auto mx = [](int u, int v, int w) { return u > v ? (u > w ? u : w) : (v > w ? v : w); };
    tx = pre < 0 ? mx(xa, xb, xc) : (pre ? xp : xb);
    ty = pre < 0 ? mx(a, b, ac) : (pre ? yp : b);
    if (pre == 0 && wide) {
        tx = ZsTile<float>::TXPOST_W;
        ty = ZsTile<float>::TYPOST_W;
    }
}

bool fused_supported(int rb, int dim, int ns, const Geo& g, const FusedTuning& tu)
{
    if (dim == 2)
        return ns == 2 && g.nz == 1 && g.nx % ys_tx(rb, g, tu) == 0 && g.ny >= 16 && g.ny % ys_rows(g, tu) == 0;
    if (dim != 3 || ns != 2) return false;
    int TX, TY;
    zs_tile(rb, TX, TY);
    return g.nx % TX == 0 && g.ny % TY == 0 && g.nz >= 16 && (g.nz & 1) == 0;
}

// planes per workgroup: halve the z-chunk until there are >= FusedTuning::wgs (default 256, one per CU)
// workgroups or a chunk would drop below 16 planes
int fused_zc(int rb, const Geo& g, bool pre, bool clz, const FusedTuning& tu)
{
    if (g.gnz == 1 && g.nz == 1) return ys_rows(g, tu);  // 2D: rows per chunk
    int TX, TY;
    zs_tile(rb, TX, TY, pre ? 1 : 0, clz, !pre && zs_wide(rb, g, clz, tu));
    const int64_t target = tu.wgs;
    const int64_t tiles = (int64_t)(g.nx / TX) * (g.ny / TY);
    int64_t chunks = 1;
    while (tiles * chunks < target && g.nz / (chunks * 2) >= 16) chunks *= 2;
    // POST: streams of at most tu.post_zc planes (planes of many tiles run as one chunk otherwise: the 4096^2 x 512
    // slab's POST 30.5 -> 28.5 ms per F-cycle with 256-plane chunks; the workgroups drift apart over long streams and
    // the y-neighbours' halo rows miss in L2)
    while (!pre && tu.post_zc > 0 && g.nz / chunks > tu.post_zc && g.nz / (chunks * 2) >= 16) chunks *= 2;
    return (int)(g.nz / chunks);
}

int fused_blocks(int rb, const Geo& g, int zc, bool clz, const FusedTuning& tu)  // POST's workgroups (err partials)
{
    if (g.gnz == 1 && g.nz == 1) return (g.nx / ys_tx(rb, g, tu)) * (g.ny / zc);
    int TX, TY;
    zs_tile(rb, TX, TY, 0, clz, zs_wide(rb, g, clz, tu));
    return (int)((int64_t)(g.nx / TX) * (g.ny / TY) * (g.nz / zc));
}

int fused_halo(bool pre) { return pre ? 5 : 4; }

bool fused_fwf_supported(int rb, int dim, bool clz, bool dist, const FusedTuning& tu)
{
    // fp32 levels without a boundary-modified operator (level 0), one rank's whole level: the fused PRE's trapezoid
    // is 6 deep with the full weighting, deeper than a slab's kZsHaloPre ghost planes; fp64 tiles would exceed the LDS;
    // 3D only (k_ys has no such variant)
    return rb == 4 && dim == 3 && clz && !dist && tu.fwf;
}

hipError_t prepare_kernels(int rb)
{
    hipError_t e = rb == 4 ? fused_attr<float, true>() : zs_attr_f64();
    if (e == hipSuccess && rb == 4) e = fused_attr<float, false>();
    if (e == hipSuccess) e = zs_split_attr(rb);
    if (e == hipSuccess) e = tail_attr(rb);
    if (e == hipSuccess) e = blk_attr(rb);
    if (e == hipSuccess) e = blk2_attr(rb);
    return e;
}

hipError_t launch_fused(int rb, const FusedArgs& a, hipStream_t s)
{
    const bool clz = a.cl == 0.0;
    if (a.g.gnz == 1 && a.g.nz == 1) return launch_fused_2d(rb, a, s);  // 2D level: k_ys
    if (rb == 4) return clz ? fused_dispatch<float, true>(a, s) : fused_dispatch<float, false>(a, s);
    return launch_fused_f64(a, s);
}

}  // namespace mgp
