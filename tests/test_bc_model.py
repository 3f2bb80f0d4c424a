"""CPU tests of the box boundaries MGP_BC_FACE (u = 0 on the face, cl = +1 on every level) and MGP_BC_NEUMANN
(du/dn = 0, cl = -1): the host model of tests/bc_model.py against the NumPy restatement of the pieces, its convergence
and second-order accuracy, the host-only plans, and the Markstein division on the new diagonals."""
import itertools
import shutil
import subprocess

import numpy as np
import pytest

import mgp_oracle_np as N
from abi_model import F as FIELD_F
from bc_model import BC_CL, BcModel, mean_free

BCS = ("face", "neumann")
RB = dict(smoother="rbgs", nu1=2, nu2=2)


def _mg():
    import mgpoisson
    return mgpoisson


def _n3(n):
    return tuple(n) + (1,) * (3 - len(n))


# ---- the model's cycle == the same cycle composed from the NumPy pieces ----

def _np_cycle(l, u, f, h, dim, cl, kw, fcycle, nlev):
    sm = N.RBGS
    if l == nlev - 1:
        if u.size == 1 and cl == -1.0:  # the singular cell
            return np.zeros_like(u)
        return N.smooth(u, f, h, dim, sm, 1 if u.size == 1 else 48, cl)
    u = N.smooth(u, f, h, dim, sm, kw["nu1"], cl)
    r = N.residual(u, f, h, dim, cl)
    R = N.restrict_fw(r, dim, cl) if kw["restriction"] == "full_weighting" else N.restrict(r, dim)
    V = np.zeros_like(R)
    if fcycle:
        V = _np_cycle(l + 1, V, R, 2 * h, dim, cl, kw, True, nlev)
    V = _np_cycle(l + 1, V, R, 2 * h, dim, cl, kw, False, nlev)
    kind = N.PROLONG_LINEAR if kw["prolong"] == "linear" else N.PROLONG_PC
    u = N.add_to(u, N.prolong(V, u.shape, dim, kind, cl))
    return N.smooth(u, f, h, dim, sm, kw["nu2"], cl)


@pytest.mark.parametrize("bc,real,box,cycle,restriction,prolong", list(itertools.product(
    BCS, ("double", "float"), ((16, 16), (8, 8, 8), (8, 8, 32)), "VF", ("average", "full_weighting"), ("linear", "pc"))))
def test_model_cycle_equals_numpy_pieces(bc, real, box, cycle, restriction, prolong):
    dim = len(box)
    kw = dict(dim=dim, n=_n3(box), real=real, cycle=cycle, restriction=restriction, prolong=prolong, coarse_bc=bc, **RB)
    m = BcModel(**kw)
    rng = np.random.default_rng(7)
    psi = rng.uniform(-1, 1, m.shapes[0]).astype(m.dtype)
    f = rng.uniform(-1, 1, m.shapes[0]).astype(m.dtype)
    if bc == "neumann":
        f = mean_free(f)
    m.u[0], m.f[0] = psi.copy(), f.copy()
    shp3 = m.shapes[0] if dim == 3 else (1,) + m.shapes[0]
    u = psi.reshape(shp3)
    for _ in range(2):
        m.cycles(1)
        u = _np_cycle(0, u, f.reshape(shp3), 1.0 / box[0], dim, BC_CL[bc], kw, cycle == "F", m.nlev)
        assert np.array_equal(m.u[0].reshape(shp3), u)
    assert np.isfinite(u).all()
    if bc == "neumann" and m.u[-1].size == 1:
        assert m.u[-1].tobytes() == np.zeros(1, m.dtype).tobytes()  # +0, all bits zero


# ---- convergence (fp64, mean-free normal f, zero start, RB-GS 2+2, linear P, average R) ----

@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("box", [(32, 32), (16, 16, 16), (8, 8, 32)])
def test_residual_falls_per_cycle(bc, box):
    dim = len(box)
    m = BcModel(dim=dim, n=_n3(box), real="double", prolong="linear", coarse_bc=bc, **RB)
    m.set_field(0, FIELD_F, mean_free(np.random.default_rng(1).standard_normal(m.shapes[0])))
    rn = [m.residual_norm(0)[0]]
    for _ in range(6):
        m.cycles(1)
        rn.append(m.residual_norm(0)[0])
    ratios = [rn[k] / rn[k - 1] for k in range(2, 7)]
    print(bc, box, ["%.3f" % r for r in ratios])
    assert max(ratios) <= 0.15, ratios


# ---- second-order accuracy against manufactured solutions ----

def _exact(bc, shape):
    fn = np.sin if bc == "face" else np.cos
    u = np.ones(shape)
    for ax, n in enumerate(shape):
        x = (np.arange(n) + 0.5) / n
        s = [1] * len(shape)
        s[ax] = n
        u = u * fn(np.pi * x).reshape(s)
    return u


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("dim,sizes", [(2, (16, 32, 64)), (3, (8, 16, 32))])
def test_second_order_accuracy(bc, dim, sizes):
    errs = []
    for n in sizes:
        m = BcModel(dim=dim, n=_n3((n,) * dim), real="double", prolong="linear", coarse_bc=bc, **RB)
        ex = _exact(bc, m.shapes[0])
        f = -dim * np.pi ** 2 * ex
        m.set_field(0, FIELD_F, mean_free(f) if bc == "neumann" else f)
        m.cycles(14)
        psi = m.u[0]
        if bc == "neumann":
            psi, ex = psi - psi.mean(), ex - ex.mean()
        errs.append(float(np.abs(psi - ex).max()))
    ratios = [errs[i] / errs[i + 1] for i in range(len(errs) - 1)]
    print(bc, dim, errs, ratios)
    assert min(ratios) >= 3.5, (errs, ratios)


# ---- the host-only plans ----

NS512 = dict(dim=3, n=(512, 512, 512), real="float", prolong="linear", **RB)


def test_plan_accepts_the_new_boundaries_and_refuses_4():
    mg = _mg()
    for bc in (2, 3):
        assert len(mg.plan(mg.make_opts(dim=3, n=(16, 16, 16), coarse_bc=bc))) == 5
        assert len(mg.plan_batch(mg.make_opts(dim=3, n=(16, 16, 16), coarse_bc=bc), 3)) == 5
    from mgpoisson.context import COARSE_BCS
    assert COARSE_BCS["face"] == 2 and COARSE_BCS["neumann"] == 3
    for bad in (4, -1):
        with pytest.raises(mg.MGPError) as ei:
            mg.plan(mg.make_opts(dim=3, n=(16, 16, 16), coarse_bc=bad))
        assert "coarse_bc" in str(ei.value)
        with pytest.raises(mg.MGPError) as ei:
            mg.plan_batch(mg.make_opts(dim=3, n=(16, 16, 16), coarse_bc=bad), 3)
        assert "coarse_bc" in str(ei.value)


def test_plan_512_engine_column_is_the_same_under_every_boundary():
    mg = _mg()
    cols = {bc: [r["engine"] for r in mg.plan(mg.make_opts(coarse_bc=bc, **NS512))] for bc in range(4)}
    assert cols[0][:2] == ["zs", "zpost"] and "blk" in cols[0] and cols[0][-1] == "tail"
    i = cols[0].index("blk")
    assert set(cols[0][2:i]) <= {"piece"} and set(cols[0][i:]) <= {"blk", "tail"}
    for bc in (1, 2, 3):
        assert cols[bc] == cols[0], (bc, cols[bc])


def test_plan_comm_face_equals_consistent():
    mg = _mg()
    kw = dict(dim=3, n=(256, 256, 64), real="float", prolong="linear", rank=0, world=2, comm_id=b"\0" * 128, **RB)
    ref = mg.plan_comm(mg.make_opts(coarse_bc=1, **kw), 2)
    assert ref and mg.plan_comm(mg.make_opts(coarse_bc=2, **kw), 2) == ref
    assert mg.plan_comm(mg.make_opts(coarse_bc=3, **kw), 2) == ref


# ---- the Markstein division on the new diagonals ----

DIV_C = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint64_t nxt(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
/* a numerator: a uniform mantissa in [1, 2) with a random sign, scaled by 2^e, e in [-24, 24] */
static double num(void)
{
    const uint64_t r = nxt();
    const double m = 1.0 + (double)(r >> 12) * (1.0 / 4503599627370496.0);
    const int e = (int)((r >> 1) % 49) - 24;
    return ldexp((r & 1) ? -m : m, e);
}
int main(void)
{
    long bad = 0, total = 0;
    for (int dim = 2; dim <= 3; ++dim)
        for (int sign = -1; sign <= 1; sign += 2)
            for (int nb = 1; nb <= 2 * dim; ++nb)
                for (int l = 0; l <= 13; ++l) {
                    const double h = ldexp(1.0, l) / 4096.0;
                    {
                        const float hs = (float)h * (float)h;
                        const float d = ((float)(-2 * dim) - (float)nb * (float)sign) / hs;
                        if (d != 0.0f) {
                            const float y = 1.0f / d;
                            long b = 0;
                            for (int i = 0; i < 1000000; ++i) {
                                const float a = (float)num();
                                const float q = a * y;
                                const float r = fmaf(-q, d, a);
                                if (fmaf(r, y, q) != a / d) ++b;
                            }
                            if (b) printf("fp32 dim %d cl %d nb %d level %d: %ld differ\n", dim, sign, nb, l, b);
                            bad += b;
                            total += 1000000;
                        }
                    }
                    {
                        const double hs = h * h;
                        const double d = ((double)(-2 * dim) - (double)nb * (double)sign) / hs;
                        if (d != 0.0) {
                            const double y = 1.0 / d;
                            long b = 0;
                            for (int i = 0; i < 1000000; ++i) {
                                const double a = num();
                                const double q = a * y;
                                const double r = fma(-q, d, a);
                                if (fma(r, y, q) != a / d) ++b;
                            }
                            if (b) printf("fp64 dim %d cl %d nb %d level %d: %ld differ\n", dim, sign, nb, l, b);
                            bad += b;
                            total += 1000000;
                        }
                    }
                }
    printf("checked %ld bad %ld\n", total, bad);
    return bad != 0;
}
"""


def test_markstein_division_equals_plain_division_on_the_new_diagonals(tmp_path):
    """Every divisor (-2 dim -+ nb) / h^2 of the two boundaries (the zero one, Neumann's one-cell level, is never
    divided by): div_rn's sequence y = RN(1/d), q = a y, r = fma(-q, d, a), fma(r, y, q) against a / d."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "div.c"
    src.write_text(DIV_C)
    exe = tmp_path / "div"
    subprocess.run([cc, "-O2", "-ffp-contract=off", "-o", str(exe), str(src), "-lm"], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    print(p.stdout[-2000:])
    assert p.returncode == 0, p.stdout[-2000:]
    # dims 2 and 3: (4 + 6) nb, two signs, less Neumann's zero diagonal per dim; 14 levels, two types, 1e6 numerators
    assert "checked %d bad 0" % (((4 + 6) * 2 - 2) * 14 * 2 * 1000000) in p.stdout

