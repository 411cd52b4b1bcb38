"""The Generalized-ICP refinement (fgoicp_gicp_terms, fgoicp_ctx_set_source_normals, fgoicp_source_normals, fgoicp_gicp_moments,
fgoicp_icp_gicp, fgoicp_solver_refine_gicp) as far as it goes without a GPU: the per-pair arithmetic the kernel shares with the host
against numpy, the refusals, a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer that recovers a known twist,
and the CLI's keys."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(REPO, "tests", "host_harness")
INVALID_ARG = 1
f32, f64 = np.float32, np.float64
TRIU3, TRIU6 = np.triu_indices(3), np.triu_indices(6)


def _msg(lib):
    return lib.fgoicp_last_error().decode()


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def skew(x):
    return np.array([[0, -x[2], x[1]], [x[2], 0, -x[0]], [-x[1], x[0], 0]], f64)


def numpy_pair(x, q, nq, np_, R, eps):
    """the definition in float64 from the float32 values: S, M = inv(S), the 28 terms, and per term the magnitude the bound applies to —
    the expansion's summands |J_a| |M_ab| |J_b| with every |M_ab| at the largest |M| entry, which is what the bound on M is relative to"""
    x, q, nq, np_, R = (np.asarray(v, f32).astype(f64) for v in (x, q, nq, np_, R))
    m = R @ np_
    S = 2 * np.eye(3) - (1 - eps) * (np.outer(nq, nq) + np.outer(m, m))
    M = np.linalg.inv(S)
    J = np.hstack([-skew(x), np.eye(3)])
    d = x - q
    v = np.concatenate([(J.T @ M @ J)[TRIU6], J.T @ M @ d, [d @ M @ d]])
    big = np.abs(M).max() * np.ones((3, 3))
    aJ, ad = np.abs(J), np.abs(d)
    mag = np.concatenate([(aJ.T @ big @ aJ)[TRIU6], aJ.T @ big @ ad, [ad @ big @ ad]])
    return S, M, v, mag


def _pairs(fg, n, seed):
    """n random pairs; the last 100: n_q = +-(R n_p) rounded to float32, the worst-conditioned S (cond S = 1 / epsilon)"""
    rng = np.random.default_rng(seed)
    x, q = rng.uniform(-1, 1, (n, 3)).astype(f32), rng.uniform(-1, 1, (n, 3)).astype(f32)
    nq, np_ = unit(rng.normal(size=(n, 3))).astype(f32), unit(rng.normal(size=(n, 3))).astype(f32)
    R = np.stack([fg.synth.random_rotation(rng).astype(f32) for _ in range(n)])
    sign = np.where(np.arange(100) % 2 == 0, 1.0, -1.0)[:, None]
    nq[-100:] = (sign * np.einsum("nij,nj->ni", R[-100:].astype(f64), np_[-100:].astype(f64))).astype(f32)
    return x, q, nq, np_, R


# ---- 1. the per-pair arithmetic against numpy ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [1.0, 1e-1, 1e-3])
def test_gicp_terms_match_numpy(fg, eps):
    """M against numpy.linalg.inv(S) within 64 (1 / eps) 2^-53 of the largest |M| entry (an adjugate inverse of a matrix of condition
    1 / eps); the 28 terms within the same factor times the magnitude of their expansion (numpy_pair)"""
    bound = 64 * (1 / eps) * 2.0 ** -53
    worst_M = worst_v = 0.0
    for x, q, nq, np_, R in zip(*_pairs(fg, 1000, 11)):
        S, M, v, mag = numpy_pair(x, q, nq, np_, R, eps)
        gM, gv = fg.gicp_terms(x, q, nq, np_, R, eps)
        assert np.array_equal(gM, gM.T)
        worst_M = max(worst_M, float(np.abs(gM - M).max() / np.abs(M).max()))
        worst_v = max(worst_v, float((np.abs(gv - v) / mag).max()))
    print(f"epsilon {eps}: largest error / bound: M {worst_M / bound:.3g}, terms {worst_v / bound:.3g}")
    assert worst_M <= bound and worst_v <= bound


@pytest.mark.parametrize("eps", [1.0, 1e-1, 1e-3])
def test_equal_normals_give_the_closed_form(fg, eps):
    """m = n_q = n: M = (I + ((1 - eps) / eps) n n^T) / 2 for a unit n.  Exactly unit float32 vectors are the axes (m = n_q exactly needs a
    rotation that is exact in float32: the signed permutations); for a generic float32 n, |n|^2 = 1 + delta, the same inverse by
    Sherman-Morrison is (I + (1 - eps) n n^T / (1 - (1 - eps) |n|^2)) / 2, which is the closed form at delta = 0"""
    bound = 64 * (1 / eps) * 2.0 ** -53
    a = 1 - eps
    worst = 0.0
    perms = [np.eye(3)[list(p)] * np.array(s)[:, None] for p in ((0, 1, 2), (1, 2, 0), (2, 0, 1)) for s in ((1, 1, 1), (-1, -1, 1), (1, -1, -1))]
    for R in perms:
        for k in range(3):
            for sgn in (1.0, -1.0):
                n_p = np.zeros(3, f32); n_p[k] = sgn
                n = (R @ n_p).astype(f32)
                gM, _ = fg.gicp_terms(np.zeros(3), np.zeros(3), n, n_p, R, eps)
                want = 0.5 * (np.eye(3) + (a / eps) * np.outer(n, n))
                worst = max(worst, float(np.abs(gM - want).max() / np.abs(want).max()))
    rng = np.random.default_rng(5)
    for _ in range(200):
        n = unit(rng.normal(size=3)).astype(f32)
        n64 = n.astype(f64)
        gM, _ = fg.gicp_terms(np.zeros(3), np.zeros(3), n, n, np.eye(3), eps)
        want = 0.5 * (np.eye(3) + a * np.outer(n64, n64) / (1 - a * (n64 @ n64)))
        worst = max(worst, float(np.abs(gM - want).max() / np.abs(want).max()))
    print(f"epsilon {eps}: largest deviation from the closed form / bound {worst / bound:.3g}")
    assert worst <= bound


def test_plane_terms_are_the_limit_and_the_terms_are_even_in_both_normals(fg):
    """flipping n_q or n_p changes nothing, bit for bit (the products are the same numbers); as eps -> 0 with m = n_q the weighted terms
    2 eps J^T M J approach the point-to-plane J^T n n^T J"""
    rng = np.random.default_rng(2)
    x, q = rng.uniform(-1, 1, 3).astype(f32), rng.uniform(-1, 1, 3).astype(f32)
    nq, np_, R = unit(rng.normal(size=3)).astype(f32), unit(rng.normal(size=3)).astype(f32), fg.synth.random_rotation(rng).astype(f32)
    M0, v0 = fg.gicp_terms(x, q, nq, np_, R)
    for a, b in ((-nq, np_), (nq, -np_), (-nq, -np_)):
        M1, v1 = fg.gicp_terms(x, q, a, b, R)
        assert M1.tobytes() == M0.tobytes() and v1.tobytes() == v0.tobytes()
    n = np.array([0.0, 0.0, 1.0], f32)
    eps = 1e-9
    _, v = fg.gicp_terms(x, q, n, n, np.eye(3), eps)
    Jn = np.concatenate([np.cross(x.astype(f64), n), n])
    r = n.astype(f64) @ (x.astype(f64) - q.astype(f64))
    plane = np.concatenate([np.outer(Jn, Jn)[TRIU6], Jn * r, [r * r]])
    assert np.abs(2 * eps * v - plane).max() <= 1e-7


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------
def test_gicp_terms_refuses_null_pointers_and_a_bad_epsilon(fg):
    lib = fg._lib.load()
    fp, dp = fg._lib.c_float_p, C.POINTER(C.c_double)
    z = np.array([0, 0, 1], f32)
    R = np.eye(3, dtype=f32).reshape(9)
    v = np.empty(28, f64)
    ok = [z.ctypes.data_as(fp)] * 4 + [R.ctypes.data_as(fp)]
    assert lib.fgoicp_gicp_terms(*ok, 1e-3, None, v.ctypes.data_as(dp)) == 0
    assert lib.fgoicp_gicp_terms(*ok, 1e-3, None, None) == 0  # both outputs are optional
    for k in range(5):
        args = list(ok)
        args[k] = None
        assert lib.fgoicp_gicp_terms(*args, 1e-3, None, v.ctypes.data_as(dp)) == INVALID_ARG and "fgoicp_gicp_terms" in _msg(lib) and "null" in _msg(lib)
    for bad in (0.0, -1.0, 1.0000001, 2.0, float("nan"), float("inf")):
        assert lib.fgoicp_gicp_terms(*ok, bad, None, v.ctypes.data_as(dp)) == INVALID_ARG and "epsilon" in _msg(lib)
    with pytest.raises(fg.FgoicpError):
        fg.gicp_terms(z, z, z, z, np.eye(3), 0.0)


def test_device_calls_refuse_null_handles_bad_structs_thresholds_and_epsilons_before_any_device_work(fg):
    lib = fg._lib.load()
    fp = fg._lib.c_float_p
    R, t = np.eye(3, dtype=f32).reshape(9), np.zeros(3, f32)
    Rp, tp = R.ctypes.data_as(fp), t.ctypes.data_as(fp)
    pm, pr = fg._lib.PlaneMoments(), fg._lib.PlaneResult()
    inf = float("inf")
    assert lib.fgoicp_ctx_set_source_normals(None, None, 16) == INVALID_ARG and "fgoicp_ctx_set_source_normals" in _msg(lib)
    assert lib.fgoicp_source_normals(None, Rp) == INVALID_ARG and "fgoicp_source_normals" in _msg(lib)
    assert lib.fgoicp_gicp_moments(None, Rp, tp, inf, 1e-3, C.byref(pm)) == INVALID_ARG and "fgoicp_gicp_moments" in _msg(lib) and "null" in _msg(lib)
    assert lib.fgoicp_icp_gicp(None, Rp, tp, 30, 1e-6, inf, 1e-3, C.byref(pr)) == INVALID_ARG and "fgoicp_icp_gicp" in _msg(lib) and "null" in _msg(lib)
    assert lib.fgoicp_solver_refine_gicp(None, 16, 30, 1e-6, inf, 1e-3, C.byref(pr)) == INVALID_ARG and "fgoicp_solver_refine_gicp" in _msg(lib)
    assert (pm.points, pm.correspondences, pr.iterations, pr.rank) == (0, 0, 0, 0)
    fake = C.c_void_p(1)  # never followed: everything below is refused before the context is looked at
    for cls, call in ((fg._lib.PlaneMoments, lambda o, d=inf, e=1e-3: lib.fgoicp_gicp_moments(fake, Rp, tp, d, e, o)),
                      (fg._lib.PlaneResult, lambda o, d=inf, e=1e-3: lib.fgoicp_icp_gicp(fake, Rp, tp, 30, 1e-6, d, e, o))):
        buf = (C.c_ubyte * 512)(*([0xA5] * 512))
        out = C.cast(buf, C.POINTER(cls))
        out.contents.struct_size = 0
        assert call(out) == INVALID_ARG and "struct_size" in _msg(lib)
        assert bytes(buf)[4:] == bytes([0xA5] * 508) and out.contents.struct_size == 0
        assert call(None) == INVALID_ARG
        ok = cls()
        for d in (float("nan"), -1.0):
            assert call(C.byref(ok), d) == INVALID_ARG and "max_dist2" in _msg(lib)
        for e in (0.0, -1.0, 2.0, float("nan")):
            assert call(C.byref(ok), inf, e) == INVALID_ARG and "epsilon" in _msg(lib)


# ---- 3. the stand-alone program under the sanitizers ----------------------------------------------------------------------------------
def test_a_known_twist_is_recovered_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "gicp_twist_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                    "-o", exe, os.path.join(HERE, "gicp_twist_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    print(p.stderr)
    assert p.returncode == 0, p.stderr[-4000:]
    assert "all checks passed" in p.stderr and p.stderr.count("largest deviation") == 3
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr and "LeakSanitizer" not in p.stderr


# ---- 4. the CLI ----------------------------------------------------------------------------------------------------------------------
class GicpConfigOut(C.Structure):
    _fields_ = [("refine", C.c_char * 64), ("error", C.c_char * 512), ("refine_knn", C.c_int), ("refine_max_iter", C.c_int), ("refine_distance", C.c_float),
                ("refine_epsilon", C.c_double)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("gicp_harness") / "libgicp_harness.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "gicp_harness.cpp")], check=True)
    L = C.CDLL(so)
    L.gicp_parse_config.argtypes = [C.c_char_p, C.POINTER(GicpConfigOut)]
    L.gicp_write_result.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p]
    return L


def test_cli_parser_reads_gicp_and_its_epsilon_and_refuses_bad_ones(harness, tmp_path):
    base = '[io]\ntarget = "t.txt"\nsource = "s.txt"\noutput = "out.toml"\n[params]\nlut_resolution = 0.01\nmse_threshold = 0.002\n{params}'

    def parse(params):
        out = GicpConfigOut()
        (tmp_path / "c.toml").write_text(base.format(params=params))
        return harness.gicp_parse_config(str(tmp_path / "c.toml").encode(), C.byref(out)), out

    rc, out = parse('refine = "gicp"\n')
    assert rc == 0 and (out.refine, out.refine_knn, out.refine_max_iter, out.refine_distance, out.refine_epsilon) == (b"gicp", 16, 30, 0.0, 1e-3)
    rc, out = parse('refine = "gicp"\nrefine_knn = 12\nrefine_max_iter = 7\nrefine_distance = 0.125\nrefine_epsilon = 0.25\n')
    assert rc == 0 and (out.refine, out.refine_knn, out.refine_max_iter, out.refine_distance, out.refine_epsilon) == (b"gicp", 12, 7, 0.125, 0.25)
    rc, out = parse('refine = "gicp"\nrefine_epsilon = 1\n')
    assert rc == 0 and out.refine_epsilon == 1.0
    rc, out = parse('refine = "plane"\nrefine_epsilon = 5\n')  # not read by "plane"
    assert rc == 0 and out.refine == b"plane"
    for bad in ("0", "-1", "2", "nan"):
        rc, out = parse(f'refine = "gicp"\nrefine_epsilon = {bad}\n')
        assert rc == 2 and b"refine_epsilon" in out.error, bad
    for params, text in (('refine = "other"\n', b'"other"'), ('refine = "gicp"\nrefine_knn = 3\n', b"refine_knn"), ('refine = "gicp"\nrefine_knn = 33\n', b"refine_knn")):
        rc, out = parse(params)
        assert rc == 2 and text in out.error, params
    rc, out = parse('refine = "other"\n')
    assert b'"plane"' in out.error and b'"gicp"' in out.error  # the message lists both refinements


def test_result_file_names_the_residual_after_the_refinement(fg, harness, tmp_path):
    raw = fg._lib.PlaneResult()
    raw.R[:] = [0, 1, 0, -1, 0, 0, 0, 0, 1]
    raw.t[:] = [0.5, -0.25, 4]
    raw.iterations, raw.rank, raw.correspondences, raw.plane_rmse, raw.scaling_factor = 9, 6, 123, 0.5, 4.0
    ptr = C.cast(C.byref(raw), C.c_void_p)
    assert harness.gicp_write_result(str(tmp_path / "plane.toml").encode(), ptr, None) == 0
    assert harness.gicp_write_result(str(tmp_path / "gicp.toml").encode(), ptr, b"gicp_rmse") == 0
    plane, gicp = (tmp_path / "plane.toml").read_text(), (tmp_path / "gicp.toml").read_text()
    assert "plane_rmse = 0.125" in plane and "gicp_rmse" not in plane
    assert gicp == plane.replace("plane_rmse = 0.125", "gicp_rmse = 0.125")
