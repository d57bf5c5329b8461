"""The step checker of itsol_steps.py has teeth: a clean working-precision model of the solvers passes it with every ratio at
most 1, and the same model with one defect fails it, for every type and at every size of the GPU test.  This is what makes the
inputs of test_gpu_itsol_steps.py meaningful: the bounds are tight enough there to see a dropped block, a dropped trip, a skipped
element or a conjugated dot."""
import numpy as np
import pytest

import itsol_steps as K

# A single-precision defect that drops exactly ONE element may stay inside the bound of the scalar it spoils; it then has to be
# caught elementwise or by the double-precision run of the same template (which is asserted for every case below).  Cases
# that need this exception, by name; every other (defect, type, size) must fail the checker outright.
SINGLE_ELEMENT_EXCEPTIONS = ()


def cg_run(prec, n, precond, iters, defect=None):
    S = K.ModelSolver(prec, n, "cg", precond, defect=defect)
    ck = K.CgCheck(prec, n, S.b, S.x, precond)
    with np.errstate(all="ignore"):
        K.drive_cg(S, ck, min(iters, n))
    return ck


def gmres_run(prec, n, precond, cycles, defect=None, ratios=None):
    S = K.ModelSolver(prec, n, "gmres", precond, restart=4, defect=defect)
    ck = K.GmresCheck(prec, n, S.b)

    def cycle(x0, x1, basis):
        if ratios is not None:
            ratios.append(K.min_residual_ratio(S.diag, S.lo, S.up, S.b, x0, x1, basis))

    with np.errstate(all="ignore"):
        K.drive_gmres(S, ck, 4, cycles, cycle)
    return ck


@pytest.mark.parametrize("n", K.SIZES)
@pytest.mark.parametrize("prec", K.PRECS)
def test_clean_model_passes(prec, n):
    for precond in (False, True):
        ck = cg_run(prec, n, precond, 6)
        assert ck.ok(), (precond, ck.report())
        assert set(ck.ratios) >= ({"rinfo[RES_NORM]", "rinfo[RHS_NORM]"} | ({"x += alpha p", "r += alpha q"} if n > 0 else set()))
    ratios = []
    ck = gmres_run(prec, n, False, 2, ratios=ratios)
    assert ck.ok(), ck.report()  # includes: the bound stays below 1e-3 max|v|, so the case checks something
    if n > 4:
        margins = K.cycle_margins(prec, n, [f for r, f in ratios])
        assert "v[j+1]" in ck.ratios and len(ratios) == 2
        assert all(r <= m for (r, f), m in zip(ratios, margins)), ([r - 1 for r, f in ratios], [m - 1 for m in margins])
    ck = gmres_run(prec, n, True, 1)
    assert ck.ok(), ck.report()


@pytest.mark.parametrize("n", K.SIZES)
@pytest.mark.parametrize("prec", K.PRECS)
def test_every_live_defect_fails(prec, n):
    seen = []
    for defect in K.DEFECTS:
        if not K.live(prec, n, defect):
            continue
        name = "%s-%s-%d" % (defect, prec, n)
        ck = cg_run(prec, n, False, 2, defect)
        if name + "-cg" in SINGLE_ELEMENT_EXCEPTIONS:
            twin = cg_run({"s": "d", "c": "z"}[prec], n, False, 2, defect)
            assert not twin.ok(), name
        else:
            assert not ck.ok(), (name, "cg", ck.report())
        if defect != "conj" and n > 4:  # (GMRES has no alpha)
            ck = gmres_run(prec, n, False, 1, defect)
            if name + "-gmres" in SINGLE_ELEMENT_EXCEPTIONS:
                assert not gmres_run({"s": "d", "c": "z"}[prec], n, False, 1, defect).ok(), name
            else:
                assert not ck.ok(), (name, "gmres", ck.report())
        seen.append(defect)
    assert "last" in seen
    r = K.Ty(prec).route(n)
    assert ("final2" in seen) == r["final2"] and ("stride" in seen) == r["stride"]


def test_routes_cover_every_path_for_every_type():
    for prec in K.PRECS:
        live = {k for n in K.SIZES for k, v in K.Ty(prec).route(n).items() if v}
        assert live == {"tail", "final2", "stride", "cap"}, (prec, live)
    assert K.Ty("s").route(131877)["stride"] and not K.Ty("c").route(131877)["stride"] and K.Ty("c").route(262949)["stride"]
    assert all(K.Ty(p).route(65829)["final2"] for p in K.PRECS)


def test_single_precision_D_is_the_longest_chain():
    t = K.Ty("s")
    assert t.D(1) == 1 + 1 + 16 and t.D(65829) == 1 + 2 + 16 and t.D(131877) == 2 + 2 + 16
    assert K.Ty("c").D(262949) == 2 + 4 + 16 and K.Ty("c").D(131877) == 1 + 3 + 16
    assert K.Ty("d").D(65829) == 65829
