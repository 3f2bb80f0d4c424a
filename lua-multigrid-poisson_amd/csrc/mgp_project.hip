// mgp_project.hip — the two operators of a MAC-grid projection on level 0's packed layout (mgp_divergence,
// mgp_gradient, mgp_project; include/mgpoisson.h has the definitions):
//   k_div<T, DIM>             f = D v: the lexicographic face arrays vx, vy, vz read once, f written packed
//   k_grad<T, DIM, SUBTRACT>  faces = G psi (or faces -= G psi): psi read packed, the face arrays written in place
//   k_div_b, k_grad_b         the same two over the members of a batch (mgp_batch_divergence, mgp_batch_gradient,
//                             mgp_batch_project): one launch over the flat list members x items, the per-item device
//                             code shared with k_div / k_grad
// Every expression in T, each operation rounded (the unit is built without contraction).
//
// Thread-to-cell mapping of the vector forms: an item is C = 2 N consecutive cells of one row (N = the reals of a 16-byte
// vector: 8 cells in fp32, 4 in fp64), BOTH colours.  Those cells are N consecutive slots of the row in the red half and
// N in the black half, so the packed side is two aligned 16-byte accesses, and the y and z face rows (nx reals, nx a
// multiple of C) are aligned 16-byte accesses too.  The x face rows hold nx + 1 reals, so no row but the first is
// 16-byte aligned and the alignment differs from row to row: they are read and written one real at a time, C + 1 of
// them per item (neighbouring items share one face; the shared face and the straddled lines come from cache).  A colour
// per item would make the packed side one vector instead of two, but read every face row twice, from workgroups half a
// plane apart.  The gradient reads psi of rows j - 1 and plane k - 1 beside its own: with the workgroups of a launch
// handed to the XCDs in contiguous bands (xcd_remap) those were loaded a row or a plane earlier by the same XCD.
// The scalar forms (rows shorter than C, nx = 1, an unaligned pointer or plane stride) run a thread per own slot
// (level_slot / slot_cell, as mgp_mean.hip does).  Pad slots, ghost planes and the empty slots of nx = 1 rows are
// neither read as cells nor written.
#include "mgp_device.h"

#include <algorithm>

namespace mgp {
namespace {

template <typename T>
struct PV {
    static constexpr int N = VN<T>::n, C = 2 * VN<T>::n, LC = sizeof(T) == 4 ? 3 : 2;  // cells per item and its log2
};

// item -> (i0, j, k): x fastest
template <typename T>
__device__ __forceinline__ void item_cell(int64_t it, const Geo& g, int& i0, int& j, int64_t& k)
{
    const int lrow = g.lx - PV<T>::LC;  // log2(items per row)
    i0 = (int)(it & (((int64_t)1 << lrow) - 1)) << PV<T>::LC;
    j = (int)((it >> lrow) & (g.ny - 1));
    k = it >> (lrow + g.ly);
}

// the C cells of an item from / to the two halves: cell i0 + 2 e + p is red slot e, cell i0 + 2 e + 1 - p black slot e
// (p = the row's parity (j + z0 + k) & 1)
template <typename T>
__device__ __forceinline__ void load_row(const T* __restrict__ u, const Geo& g, int i0, int j, int64_t k, T (&E)[PV<T>::C])
{
    constexpr int N = PV<T>::N;
    const int p = (int)((j + g.z0 + k) & 1);
    const T* r = u + k * g.P + (int64_t)j * g.hw + (i0 >> 1);
    const Vec<T, N> R = vload<T, N>(r), B = vload<T, N>(r + g.H);
#pragma unroll
    for (int e = 0; e < N; ++e) {
        E[2 * e] = p ? B.v[e] : R.v[e];
        E[2 * e + 1] = p ? R.v[e] : B.v[e];
    }
}

template <typename T>
__device__ __forceinline__ void load_lex(const T* __restrict__ p, T (&a)[PV<T>::C])
{
    constexpr int N = PV<T>::N;
    const Vec<T, N> lo = vload<T, N>(p), hi = vload<T, N>(p + N);
#pragma unroll
    for (int e = 0; e < N; ++e) {
        a[e] = lo.v[e];
        a[N + e] = hi.v[e];
    }
}

template <typename T>
__device__ __forceinline__ void store_lex(T* __restrict__ p, const T (&a)[PV<T>::C])
{
    constexpr int N = PV<T>::N;
    Vec<T, N> lo, hi;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        lo.v[e] = a[e];
        hi.v[e] = a[N + e];
    }
    vstore<T, N>(p, lo);
    vstore<T, N>(p + N, hi);
}

// ---- divergence --------------------------------------------------------------------------------

template <typename T, int DIM>
__device__ __forceinline__ T div_cell(const T* __restrict__ vx, const T* __restrict__ vy, const T* __restrict__ vz,
                                      const Geo& g, int i, int j, int64_t k, T ih)
{
    const int64_t nx = g.nx, ny = g.ny;
    const T* x = vx + (k * ny + j) * (nx + 1) + i;
    const T* y = vy + (k * (ny + 1) + j) * nx + i;
    T s = (x[1] - x[0]) + (y[nx] - y[0]);
    if (DIM == 3) {
        const T* z = vz + (k * ny + j) * nx + i;
        s = s + (z[nx * ny] - z[0]);
    }
    return s * ih;
}

// one item of the vector form: the C cells of item `it` of the box g (faces and f of that box)
template <typename T, int DIM>
__device__ __forceinline__ void div_item(const T* __restrict__ vx, const T* __restrict__ vy, const T* __restrict__ vz,
                                         T* __restrict__ f, const Geo& g, T ih, int64_t it)
{
    constexpr int N = PV<T>::N, C = PV<T>::C;
    const int64_t nx = g.nx, ny = g.ny;
    int i0, j;
    int64_t k;
    item_cell<T>(it, g, i0, j, k);
    const T* x = vx + (k * ny + j) * (nx + 1) + i0;
    T xs[C + 1], y0[C], y1[C], d[C];
#pragma unroll
    for (int e = 0; e <= C; ++e) xs[e] = x[e];
    const T* y = vy + (k * (ny + 1) + j) * nx + i0;
    load_lex<T>(y, y0);
    load_lex<T>(y + nx, y1);
#pragma unroll
    for (int e = 0; e < C; ++e) d[e] = (xs[e + 1] - xs[e]) + (y1[e] - y0[e]);
    if (DIM == 3) {
        const T* z = vz + (k * ny + j) * nx + i0;
        T z0[C], z1[C];
        load_lex<T>(z, z0);
        load_lex<T>(z + nx * ny, z1);
#pragma unroll
        for (int e = 0; e < C; ++e) d[e] = d[e] + (z1[e] - z0[e]);
    }
    const int p = (int)((j + g.z0 + k) & 1);
    Vec<T, N> R, B;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const T a = d[2 * e] * ih, b = d[2 * e + 1] * ih;
        R.v[e] = p ? b : a;
        B.v[e] = p ? a : b;
    }
    T* o = f + k * g.P + (int64_t)j * g.hw + (i0 >> 1);
    vstore<T, N>(o, R);
    vstore<T, N>(o + g.H, B);
}

// the scalar form's work item: the cell of packed slot o, if it holds one
template <typename T, int DIM>
__device__ __forceinline__ void div_slot(const T* __restrict__ vx, const T* __restrict__ vy, const T* __restrict__ vz,
                                         T* __restrict__ f, const Geo& g, T ih, int64_t o)
{
    int i, j;
    int64_t k;
    if (slot_cell(o, g, i, j, k)) f[o] = div_cell<T, DIM>(vx, vy, vz, g, i, j, k, ih);
}

template <typename T, int DIM, bool VEC>
__global__ __launch_bounds__(kBlock) void k_div(const T* __restrict__ vx, const T* __restrict__ vy,
                                                const T* __restrict__ vz, T* __restrict__ f, Geo g, T ih)
{
    const int64_t step = (int64_t)gridDim.x * kBlock;
    const int64_t first = (int64_t)xcd_remap((int)blockIdx.x, (int)gridDim.x) * kBlock + threadIdx.x;
    if (VEC) {
        const int64_t items = ((int64_t)g.nx * g.ny * g.nz) >> PV<T>::LC;
        for (int64_t it = first; it < items; it += step) div_item<T, DIM>(vx, vy, vz, f, g, ih, it);
    } else {
        const int64_t n = 2 * g.H * g.nz;
        for (int64_t c = first; c < n; c += step)
            div_slot<T, DIM>(vx, vy, vz, f, g, ih, level_slot(c, g.lhw + g.ly + 1, g.P));
    }
}

// The members of a batch (mgp_batch.hip): the box g is ONE member (z0 = 0, P = 2 H: no ghost planes, no pad slots),
// member m's packed field starts m << ls reals after f, its face arrays m * sx / sy / sz reals after vx / vy / vz.  The
// work of a launch is the flat list members x items (VEC: an item is C cells, 1 << lw per member; otherwise a packed
// slot, lw = ls): the member is a shift of the flat index, so a workgroup covers as many members as its threads reach.
struct BFace {
    int64_t sx, sy, sz;  // reals per member of the x / y / z face arrays
    int ls, lw;          // log2 of a member's packed slots / of its work items
};

template <typename T, int DIM, bool VEC>
__global__ __launch_bounds__(kBlock) void k_div_b(const T* __restrict__ vx, const T* __restrict__ vy,
                                                  const T* __restrict__ vz, T* __restrict__ f, Geo g, T ih, BFace bf,
                                                  int64_t total)
{
    const int64_t step = (int64_t)gridDim.x * kBlock;
    const int64_t first = (int64_t)xcd_remap((int)blockIdx.x, (int)gridDim.x) * kBlock + threadIdx.x;
    const int64_t mask = ((int64_t)1 << bf.lw) - 1;
    for (int64_t q = first; q < total; q += step) {
        const int64_t m = q >> bf.lw, w = q & mask;
        const T* x = vx + m * bf.sx;
        const T* y = vy + m * bf.sy;
        const T* z = DIM == 3 ? vz + m * bf.sz : vz;
        T* fm = f + (m << bf.ls);
        if (VEC) div_item<T, DIM>(x, y, z, fm, g, ih, w);
        else div_slot<T, DIM>(x, y, z, fm, g, ih, w);
    }
}

// ---- gradient ----------------------------------------------------------------------------------

template <typename T, bool SUBTRACT>
__device__ __forceinline__ void face_out(T* __restrict__ p, T gv)
{
    *p = SUBTRACT ? *p - gv : gv;
}

template <typename T, bool SUBTRACT>
__device__ __forceinline__ void face_out_lex(T* __restrict__ p, const T (&hi)[PV<T>::C], const T (&lo)[PV<T>::C], T ih)
{
    constexpr int C = PV<T>::C;
    T o[C];
    if (SUBTRACT) load_lex<T>(p, o);
#pragma unroll
    for (int e = 0; e < C; ++e) {
        const T gv = (hi[e] - lo[e]) * ih;
        o[e] = SUBTRACT ? o[e] - gv : gv;
    }
    store_lex<T>(p, o);
}

template <typename T, int DIM, bool SUBTRACT>
__device__ __forceinline__ void grad_item(const T* __restrict__ u, T* __restrict__ vx, T* __restrict__ vy,
                                          T* __restrict__ vz, const Geo& g, T ih, T mc, int64_t it)
{
    constexpr int C = PV<T>::C;
    const int64_t nx = g.nx, ny = g.ny;
    int i0, j;
    int64_t k;
    item_cell<T>(it, g, i0, j, k);
    T E[C], L[C], G[C];
    load_row<T>(u, g, i0, j, k, E);
    // x: the left neighbour is the odd cell i0 - 1, slot (i0 >> 1) - 1 of the half whose colour has odd cells
    {
        const int p = (int)((j + g.z0 + k) & 1);
        T left;
        if (i0 > 0) left = u[k * g.P + (int64_t)(1 - p) * g.H + (int64_t)j * g.hw + (i0 >> 1) - 1];
        else left = mc * E[0];
        T* x = vx + (k * ny + j) * (nx + 1) + i0;
        face_out<T, SUBTRACT>(x, (E[0] - left) * ih);
#pragma unroll
        for (int e = 1; e < C; ++e) face_out<T, SUBTRACT>(x + e, (E[e] - E[e - 1]) * ih);
        if (i0 + C == g.nx) face_out<T, SUBTRACT>(x + C, (mc * E[C - 1] - E[C - 1]) * ih);
    }
#pragma unroll
    for (int e = 0; e < C; ++e) G[e] = mc * E[e];
    {
        T* y = vy + (k * (ny + 1) + j) * nx + i0;
        if (j > 0) load_row<T>(u, g, i0, j - 1, k, L);
        else {
#pragma unroll
            for (int e = 0; e < C; ++e) L[e] = G[e];
        }
        face_out_lex<T, SUBTRACT>(y, E, L, ih);
        if (j == g.ny - 1) face_out_lex<T, SUBTRACT>(y + nx, G, E, ih);
    }
    if (DIM == 3) {
        T* z = vz + (k * ny + j) * nx + i0;
        if (k > 0) load_row<T>(u, g, i0, j, k - 1, L);
        else {
#pragma unroll
            for (int e = 0; e < C; ++e) L[e] = G[e];
        }
        face_out_lex<T, SUBTRACT>(z, E, L, ih);
        if (k == g.nz - 1) face_out_lex<T, SUBTRACT>(z + nx * ny, G, E, ih);
    }
}

template <typename T, int DIM, bool SUBTRACT>
__device__ __forceinline__ void grad_slot(const T* __restrict__ u, T* __restrict__ vx, T* __restrict__ vy,
                                          T* __restrict__ vz, const Geo& g, T ih, T mc, int64_t o)
{
    const int64_t nx = g.nx, ny = g.ny;
    int i, j;
    int64_t k;
    if (!slot_cell(o, g, i, j, k)) return;
    const T e = u[o], gh = mc * e;
    {
        T* x = vx + (k * ny + j) * (nx + 1) + i;
        const T lo = i > 0 ? u[pidx(g, i - 1, j, k)] : gh;
        face_out<T, SUBTRACT>(x, (e - lo) * ih);
        if (i == g.nx - 1) face_out<T, SUBTRACT>(x + 1, (gh - e) * ih);
    }
    {
        T* y = vy + (k * (ny + 1) + j) * nx + i;
        const T lo = j > 0 ? u[pidx(g, i, j - 1, k)] : gh;
        face_out<T, SUBTRACT>(y, (e - lo) * ih);
        if (j == g.ny - 1) face_out<T, SUBTRACT>(y + nx, (gh - e) * ih);
    }
    if (DIM == 3) {
        T* z = vz + (k * ny + j) * nx + i;
        const T lo = k > 0 ? u[pidx(g, i, j, k - 1)] : gh;
        face_out<T, SUBTRACT>(z, (e - lo) * ih);
        if (k == g.nz - 1) face_out<T, SUBTRACT>(z + nx * ny, (gh - e) * ih);
    }
}

template <typename T, int DIM, bool SUBTRACT, bool VEC>
__global__ __launch_bounds__(kBlock) void k_grad(const T* __restrict__ u, T* __restrict__ vx, T* __restrict__ vy,
                                                 T* __restrict__ vz, Geo g, T ih, T mc)
{
    const int64_t step = (int64_t)gridDim.x * kBlock;
    const int64_t first = (int64_t)xcd_remap((int)blockIdx.x, (int)gridDim.x) * kBlock + threadIdx.x;
    if (VEC) {
        const int64_t items = ((int64_t)g.nx * g.ny * g.nz) >> PV<T>::LC;
        for (int64_t it = first; it < items; it += step) grad_item<T, DIM, SUBTRACT>(u, vx, vy, vz, g, ih, mc, it);
    } else {
        const int64_t n = 2 * g.H * g.nz;
        for (int64_t c = first; c < n; c += step)
            grad_slot<T, DIM, SUBTRACT>(u, vx, vy, vz, g, ih, mc, level_slot(c, g.lhw + g.ly + 1, g.P));
    }
}

// k_grad over the members of a batch (k_div_b's mapping).  A member's left, row j - 1 and plane k - 1 neighbours are
// taken inside its own box (grad_item / grad_slot test i, j, k of the member): at i = 0, j = 0, k = 0 the ghost, never
// the last slots of the member before it.
template <typename T, int DIM, bool SUBTRACT, bool VEC>
__global__ __launch_bounds__(kBlock) void k_grad_b(const T* __restrict__ u, T* __restrict__ vx, T* __restrict__ vy,
                                                   T* __restrict__ vz, Geo g, T ih, T mc, BFace bf, int64_t total)
{
    const int64_t step = (int64_t)gridDim.x * kBlock;
    const int64_t first = (int64_t)xcd_remap((int)blockIdx.x, (int)gridDim.x) * kBlock + threadIdx.x;
    const int64_t mask = ((int64_t)1 << bf.lw) - 1;
    for (int64_t q = first; q < total; q += step) {
        const int64_t m = q >> bf.lw, w = q & mask;
        T* x = vx + m * bf.sx;
        T* y = vy + m * bf.sy;
        T* z = DIM == 3 ? vz + m * bf.sz : vz;
        const T* um = u + (m << bf.ls);
        if (VEC) grad_item<T, DIM, SUBTRACT>(um, x, y, z, g, ih, mc, w);
        else grad_slot<T, DIM, SUBTRACT>(um, x, y, z, g, ih, mc, w);
    }
}

// rows of whole items, and every vector access 16-byte aligned (the x faces are accessed one real at a time)
template <typename T>
bool proj_vec(int dim, const void* packed, const void* vy, const void* vz, const Geo& g)
{
    constexpr int N = PV<T>::N;
    const auto al = [](const void* p) { return (uintptr_t)p % 16 == 0; };
    return g.nx >= PV<T>::C && g.P % N == 0 && al(packed) && al(vy) && (dim == 2 || al(vz));
}

template <typename T>
unsigned proj_blocks(const Geo& g, bool vec)
{
    return nblk_gs(vec ? ((int64_t)g.nx * g.ny * g.nz) / PV<T>::C : 2 * g.H * g.nz);
}

template <typename T>
void div_t(int dim, const void* vx, const void* vy, const void* vz, void* f, const Geo& g, hipStream_t s)
{
    const bool vec = proj_vec<T>(dim, f, vy, vz, g);
    const unsigned nb = proj_blocks<T>(g, vec);
    const T ih = (T)g.nx;
    const T *x = (const T*)vx, *y = (const T*)vy, *z = (const T*)vz;
    if (dim == 3) {
        if (vec) k_div<T, 3, true><<<nb, kBlock, 0, s>>>(x, y, z, (T*)f, g, ih);
        else k_div<T, 3, false><<<nb, kBlock, 0, s>>>(x, y, z, (T*)f, g, ih);
    } else {
        if (vec) k_div<T, 2, true><<<nb, kBlock, 0, s>>>(x, y, z, (T*)f, g, ih);
        else k_div<T, 2, false><<<nb, kBlock, 0, s>>>(x, y, z, (T*)f, g, ih);
    }
}

template <typename T, int DIM, bool SUB>
void grad_ds(const void* u, void* vx, void* vy, void* vz, const Geo& g, double cl, hipStream_t s)
{
    const bool vec = proj_vec<T>(DIM, u, vy, vz, g);
    const unsigned nb = proj_blocks<T>(g, vec);
    const T ih = (T)g.nx, mc = -(T)cl;
    if (vec) k_grad<T, DIM, SUB, true><<<nb, kBlock, 0, s>>>((const T*)u, (T*)vx, (T*)vy, (T*)vz, g, ih, mc);
    else k_grad<T, DIM, SUB, false><<<nb, kBlock, 0, s>>>((const T*)u, (T*)vx, (T*)vy, (T*)vz, g, ih, mc);
}

template <typename T>
void grad_t(int dim, bool sub, const void* u, void* vx, void* vy, void* vz, const Geo& g, double cl, hipStream_t s)
{
    if (dim == 3) {
        if (sub) grad_ds<T, 3, true>(u, vx, vy, vz, g, cl, s);
        else grad_ds<T, 3, false>(u, vx, vy, vz, g, cl, s);
    } else {
        if (sub) grad_ds<T, 2, true>(u, vx, vy, vz, g, cl, s);
        else grad_ds<T, 2, false>(u, vx, vy, vz, g, cl, s);
    }
}

// ---- the members of a batch ---------------------------------------------------------------------

inline int log2_exact(int64_t v)
{
    int l = 0;
    while (((int64_t)1 << l) < v) ++l;
    return ((int64_t)1 << l) == v ? l : -1;
}

// The member strides and shifts of a launch, and whether it takes the vector form: proj_vec's conditions on the first
// member, and member strides of the packed field and of the vy / vz arrays that are multiples of 16 bytes (then every
// member's vector accesses are aligned as the first member's are).  false: g is no member box.
template <typename T>
bool batch_plan(int dim, const void* packed, const void* vy, const void* vz, const Geo& g, BFace& bf, bool& vec)
{
    constexpr int N = PV<T>::N;
    const int64_t nx = g.nx, ny = g.ny, nz = dim == 3 ? g.nz : 1, slots = g.P * g.nz;
    bf.sx = (nx + 1) * ny * nz;
    bf.sy = nx * (ny + 1) * nz;
    bf.sz = dim == 3 ? nx * ny * (nz + 1) : 0;
    bf.ls = log2_exact(slots);
    if (bf.ls < 0 || g.P != 2 * g.H || g.z0 != 0 || (dim == 2 && g.nz != 1)) return false;
    vec = proj_vec<T>(dim, packed, vy, vz, g) && slots % N == 0 && bf.sy % N == 0 && (dim == 2 || bf.sz % N == 0);
    bf.lw = vec ? log2_exact((nx * ny * nz) >> PV<T>::LC) : bf.ls;
    return bf.lw >= 0;
}

template <typename T>
hipError_t div_bt(int dim, const void* vx, const void* vy, const void* vz, void* f, const Geo& g, int nm, hipStream_t s)
{
    BFace bf;
    bool vec = false;
    if (nm < 1 || !batch_plan<T>(dim, f, vy, vz, g, bf, vec)) return hipErrorInvalidValue;
    const int64_t total = (int64_t)nm << bf.lw;
    const unsigned nb = nblk_gs(total);
    const T ih = (T)g.nx;
    const T *x = (const T*)vx, *y = (const T*)vy, *z = (const T*)vz;
    if (dim == 3) {
        if (vec) k_div_b<T, 3, true><<<nb, kBlock, 0, s>>>(x, y, z, (T*)f, g, ih, bf, total);
        else k_div_b<T, 3, false><<<nb, kBlock, 0, s>>>(x, y, z, (T*)f, g, ih, bf, total);
    } else {
        if (vec) k_div_b<T, 2, true><<<nb, kBlock, 0, s>>>(x, y, z, (T*)f, g, ih, bf, total);
        else k_div_b<T, 2, false><<<nb, kBlock, 0, s>>>(x, y, z, (T*)f, g, ih, bf, total);
    }
    return hipGetLastError();
}

template <typename T, int DIM, bool SUB>
hipError_t grad_bds(const void* u, void* vx, void* vy, void* vz, const Geo& g, double cl, int nm, hipStream_t s)
{
    BFace bf;
    bool vec = false;
    if (nm < 1 || !batch_plan<T>(DIM, u, vy, vz, g, bf, vec)) return hipErrorInvalidValue;
    const int64_t total = (int64_t)nm << bf.lw;
    const unsigned nb = nblk_gs(total);
    const T ih = (T)g.nx, mc = -(T)cl;
    if (vec) k_grad_b<T, DIM, SUB, true><<<nb, kBlock, 0, s>>>((const T*)u, (T*)vx, (T*)vy, (T*)vz, g, ih, mc, bf, total);
    else k_grad_b<T, DIM, SUB, false><<<nb, kBlock, 0, s>>>((const T*)u, (T*)vx, (T*)vy, (T*)vz, g, ih, mc, bf, total);
    return hipGetLastError();
}

template <typename T>
hipError_t grad_bt(int dim, bool sub, const void* u, void* vx, void* vy, void* vz, const Geo& g, double cl, int nm,
                   hipStream_t s)
{
    if (dim == 3) return sub ? grad_bds<T, 3, true>(u, vx, vy, vz, g, cl, nm, s) : grad_bds<T, 3, false>(u, vx, vy, vz, g, cl, nm, s);
    return sub ? grad_bds<T, 2, true>(u, vx, vy, vz, g, cl, nm, s) : grad_bds<T, 2, false>(u, vx, vy, vz, g, cl, nm, s);
}

}  // namespace

hipError_t launch_divergence(int rb, int dim, const void* vx, const void* vy, const void* vz, void* f, Geo g, hipStream_t s)
{
    MGP_REAL(rb, (div_t<T>(dim, vx, vy, vz, f, g, s)));
    return hipGetLastError();
}

hipError_t launch_gradient(int rb, int dim, bool subtract, const void* u, void* vx, void* vy, void* vz, Geo g, double cl,
                           hipStream_t s)
{
    MGP_REAL(rb, (grad_t<T>(dim, subtract, u, vx, vy, vz, g, cl, s)));
    return hipGetLastError();
}

hipError_t launch_divergence_batch(int rb, int dim, const void* vx, const void* vy, const void* vz, void* f, Geo g, int nm,
                                   hipStream_t s)
{
    MGP_REAL(rb, return (div_bt<T>(dim, vx, vy, vz, f, g, nm, s)));
    return hipErrorInvalidValue;
}

hipError_t launch_gradient_batch(int rb, int dim, bool subtract, const void* u, void* vx, void* vy, void* vz, Geo g, double cl,
                                 int nm, hipStream_t s)
{
    MGP_REAL(rb, return (grad_bt<T>(dim, subtract, u, vx, vy, vz, g, cl, nm, s)));
    return hipErrorInvalidValue;
}

}  // namespace mgp
