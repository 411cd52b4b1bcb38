"""CPU: the host half of the robust losses — fgoicp_robust_weight against the five formulas in numpy float64, bit for
bit; the layout of fgoicp_robust_moments_t / fgoicp_robust_result_t from C; the refusals that need no device; the CLI's two keys; the C++
façade's methods."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64 = np.float64
INVALID_ARG = 1
LOSSES = ("huber", "cauchy", "geman_mcclure", "tukey")
MOMENTS_FIELDS = ["struct_size", "points", "correspondences", "m", "weight_sum", "max_dist2", "loss", "scale"]
RESULT_FIELDS = ["struct_size", "R", "t", "iterations", "rank", "correspondences", "weight_sum", "rmse", "sse", "scaling_factor", "loss", "scale_estimated", "scale"]


def numpy_weight(loss, s, c):
    """the five formulas of include/fgoicp_amd.h in float64, one rounding per operation"""
    s, c = np.asarray(s, f64), f64(c)
    a = np.abs(s)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        if loss == "none":
            return np.ones_like(s)
        if loss == "huber":
            return np.where(a <= c, f64(1.0), c / np.where(a <= c, f64(1.0), a))
        if loss == "cauchy":
            u = s / c
            return f64(1.0) / (f64(1.0) + u * u)
        if loss == "geman_mcclure":
            c2 = c * c
            g = c2 / (c2 + s * s)
            return g * g
        if loss == "tukey":
            v = f64(1.0) - (s / c) * (s / c)
            return np.where(a <= c, v * v, f64(0.0))
    raise ValueError(loss)


def _bits(a):
    return np.ascontiguousarray(a, f64).view(np.uint64)


@pytest.mark.parametrize("c", [1.0, 0.00984, 0.1016, 3.7e-5, 1e-12])
def test_the_weight_is_the_numpy_formula_bit_for_bit(fg, c):
    rng = np.random.default_rng(11)
    up, down = np.nextafter(f64(c), np.inf), np.nextafter(f64(c), -np.inf)
    s = np.concatenate([[0.0, c, -c, up, -up, down, -down, 5e-324, -2.5e-310, 1e300, -1e300],
                        rng.normal(size=500) * c, rng.uniform(-4, 4, 300) * c, rng.normal(size=200) * 1e3 * c]).astype(f64)
    assert len(s) == 11 + 1000
    for loss in LOSSES:
        got = np.array([fg.robust_weight(loss, float(x), c) for x in s], f64)
        want = numpy_weight(loss, s, c)
        assert np.array_equal(_bits(got), _bits(want)), (loss, s[_bits(got) != _bits(want)][:5])
        assert ((got >= 0) & (got <= 1)).all() and got[0] == 1.0
    assert all(fg.robust_weight("none", float(x), c) == 1.0 for x in s[:20]) and fg.robust_weight(None, 3.0, -1.0) == 1.0  # no scale needed
    # continuity at c: Huber is 1 up to c and a rounding below it just beyond; Tukey falls to exactly 0 beyond c and is tiny just inside
    assert fg.robust_weight("huber", c, c) == 1.0 and fg.robust_weight("huber", down, c) == 1.0
    assert 1.0 - 4 * np.finfo(f64).eps <= fg.robust_weight("huber", up, c) < 1.0
    assert fg.robust_weight("tukey", c, c) == 0.0 and fg.robust_weight("tukey", up, c) == 0.0 and fg.robust_weight("tukey", -up, c) == 0.0
    assert 0.0 < fg.robust_weight("tukey", down, c) <= (8 * np.finfo(f64).eps) ** 2
    assert fg.robust_weight("tukey", 1e300, c) == 0.0 and fg.robust_weight("cauchy", 1e300, c) == 0.0 and fg.robust_weight("geman_mcclure", -1e300, c) == 0.0


def test_every_refusal_leaves_the_weight_untouched(fg):
    lib = fg._lib.load()
    w = C.c_double(7.0)
    bad = [(5, 0.1, 1.0), (-1, 0.1, 1.0), (1, np.nan, 1.0), (2, np.inf, 1.0), (0, -np.inf, 1.0), (1, 0.1, 0.0), (3, 0.1, -1.0), (4, 0.1, np.nan), (2, 0.1, np.inf)]
    for loss, s, c in bad:
        assert lib.fgoicp_robust_weight(loss, s, c, C.byref(w)) == INVALID_ARG and "fgoicp_robust_weight" in lib.fgoicp_last_error().decode(), (loss, s, c)
        assert w.value == 7.0
    assert lib.fgoicp_robust_weight(1, 0.1, 1.0, None) == INVALID_ARG
    assert lib.fgoicp_robust_weight(0, 0.1, np.nan, C.byref(w)) == 0 and w.value == 1.0  # none ignores the scale
    with pytest.raises(ValueError):
        fg.robust_weight("welsch", 0.1, 1.0)
    with pytest.raises(fg.FgoicpError) as e:
        fg.robust_weight("huber", 0.1, 0.0)
    assert e.value.status == INVALID_ARG and "scale" in str(e.value)


def test_the_library_exports_the_calls_and_the_structs_are_the_headers(fg, tmp_path):
    lib = fg._lib.load()
    names = ("fgoicp_robust_weight", "fgoicp_robust_moments", "fgoicp_robust_residuals", "fgoicp_robust_scale", "fgoicp_icp_robust", "fgoicp_solver_refine_robust")
    for path in (fg.build.DEFAULT_LIB, fg.build.DEV_LIB):  # the shipped library and the development build
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        for name in names:
            assert f" T {name}\n" in out, (path, name)
    for name in names:
        assert hasattr(lib, name) and name in fg._lib.exported_symbols()
    assert lib.fgoicp_abi_version() == 2
    M, R = fg._lib.RobustMoments, fg._lib.RobustResult
    assert [n for n, _ in M._fields_] == MOMENTS_FIELDS and [n for n, _ in R._fields_] == RESULT_FIELDS
    args = (["sizeof(fgoicp_robust_moments_t)"] + [f"offsetof(fgoicp_robust_moments_t, {f})" for f in MOMENTS_FIELDS] + ["sizeof(fgoicp_robust_result_t)"]
            + [f"offsetof(fgoicp_robust_result_t, {f})" for f in RESULT_FIELDS]
            + ["FGOICP_LOSS_NONE", "FGOICP_LOSS_HUBER", "FGOICP_LOSS_CAUCHY", "FGOICP_LOSS_GEMAN_MCCLURE", "FGOICP_LOSS_TUKEY", "FGOICP_MODEL_PLANE", "FGOICP_MODEL_GICP",
               "FGOICP_ABI_VERSION"])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fgoicp_amd.h"\nint main(void) { printf("' + " ".join(["%zu"] * len(args)) + '\\n", '
                   + ", ".join(f"(size_t)({a})" for a in args) + "); return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(REPO, "include"), "-o", str(tmp_path / "layout"), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(M)] + [getattr(M, f).offset for f in MOMENTS_FIELDS] + [C.sizeof(R)] + [getattr(R, f).offset for f in RESULT_FIELDS] + [0, 1, 2, 3, 4, 0, 1, 2]
    assert got == want
    assert C.sizeof(M) == 272 and C.sizeof(R) == 112 and M().struct_size == 272 and R().struct_size == 112
    assert fg._lib.LOSSES == {"none": 0, "huber": 1, "cauchy": 2, "geman_mcclure": 3, "tukey": 4}


def test_null_arguments_and_short_structs_are_refused_before_any_device_work(fg):
    """the checks in front of the context: a null context, pose or output, and a struct_size of 0 or below the size field itself"""
    lib = fg._lib.load()
    fp = fg._lib.c_float_p
    R = np.eye(3, dtype=np.float32).ravel(); t = np.zeros(3, np.float32)
    Rp, tp = R.ctypes.data_as(fp), t.ctypes.data_as(fp)
    m, r = fg._lib.RobustMoments(), fg._lib.RobustResult()
    s = C.c_double(5.0)
    fake = C.c_void_p(1)  # never dereferenced: the refusals below come first
    assert lib.fgoicp_robust_moments(None, Rp, tp, 1.0, 0, 1e-3, 1, 0.1, C.byref(m)) == INVALID_ARG and "null" in lib.fgoicp_last_error().decode()
    assert lib.fgoicp_robust_residuals(None, Rp, tp, 1.0, 0, 1e-3, 1, 0.1, None, None, None) == INVALID_ARG
    assert lib.fgoicp_robust_scale(None, Rp, tp, 1.0, 0, 1e-3, C.byref(s)) == INVALID_ARG and lib.fgoicp_robust_scale(fake, Rp, tp, 1.0, 0, 1e-3, None) == INVALID_ARG
    assert lib.fgoicp_icp_robust(None, Rp, tp, 5, 1e-6, 1.0, 0, 1e-3, 1, 0.1, C.byref(r)) == INVALID_ARG
    assert lib.fgoicp_icp_robust(fake, None, tp, 5, 1e-6, 1.0, 0, 1e-3, 1, 0.1, C.byref(r)) == INVALID_ARG
    assert lib.fgoicp_solver_refine_robust(None, 0, 16, 5, 1e-6, 1.0, 1e-3, 1, 0.0, C.byref(r)) == INVALID_ARG
    for size in (0, 3):
        m.struct_size = size; r.struct_size = size
        assert lib.fgoicp_robust_moments(fake, Rp, tp, 1.0, 0, 1e-3, 1, 0.1, C.byref(m)) == INVALID_ARG and "struct_size" in lib.fgoicp_last_error().decode()
        assert lib.fgoicp_icp_robust(fake, Rp, tp, 5, 1e-6, 1.0, 0, 1e-3, 1, 0.1, C.byref(r)) == INVALID_ARG and "struct_size" in lib.fgoicp_last_error().decode()
        assert m.struct_size == size and r.struct_size == size
    assert lib.fgoicp_robust_moments(fake, Rp, tp, 1.0, 0, 1e-3, 1, 0.1, None) == INVALID_ARG and lib.fgoicp_icp_robust(fake, Rp, tp, 5, 1e-6, 1.0, 0, 1e-3, 1, 0.1, None) == INVALID_ARG
    assert s.value == 5.0


# ---- the CLI's keys ----

@pytest.fixture(scope="module")
def config_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("robust_config") / "robust_config_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), os.path.join(REPO, "tests", "host_harness", "robust_config_check.cpp")], check=True)

    def run(tmp_path, params):
        (tmp_path / "c.toml").write_text(f'[io]\ntarget = "t.txt"\nsource = "s.txt"\n[params]\nseed = 1\n{params}')
        p = subprocess.run([str(exe), str(tmp_path / "c.toml")], capture_output=True, text=True, timeout=60)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith(("ROBUST ", "REFUSED "))]
        return p.returncode, line[-1] if line else p.stdout + p.stderr
    return run


def test_the_config_parser_reads_the_two_keys(config_check, tmp_path):
    assert config_check(tmp_path, "") == (0, "ROBUST - none 0 0")
    assert config_check(tmp_path, 'refine = "plane"\n') == (0, "ROBUST plane none 0 0")
    assert config_check(tmp_path, 'refine_loss = "none"\n') == (0, "ROBUST - none 0 0")  # no loss: params.refine is not needed
    for code, name in enumerate(LOSSES, start=1):
        for model in ("plane", "gicp"):
            assert config_check(tmp_path, f'refine = "{model}"\nrefine_loss = "{name}"\n') == (0, f"ROBUST {model} {name} {code} 0")
    assert config_check(tmp_path, 'refine = "gicp"\nrefine_loss = "tukey"\nrefine_loss_scale = 0.0125\n') == (0, "ROBUST gicp tukey 4 0.012500000000000001")
    for scale in ("0", "-1.5", "0.0"):  # a non-positive scale: estimated
        assert config_check(tmp_path, f'refine = "plane"\nrefine_loss = "huber"\nrefine_loss_scale = {scale}\n') == (0, "ROBUST plane huber 1 0")
    for bad in ("Tukey", "welsch", "l2", ""):
        rc, line = config_check(tmp_path, f'refine = "plane"\nrefine_loss = "{bad}"\n')
        assert rc == 2 and line.startswith("REFUSED") and "refine_loss" in line and "geman_mcclure" in line, line
    rc, line = config_check(tmp_path, 'refine_loss = "huber"\n')  # a loss without a refinement
    assert rc == 2 and line.startswith("REFUSED") and "params.refine" in line
    rc, line = config_check(tmp_path, 'refine = "point"\nrefine_loss = "huber"\n')
    assert rc == 2 and "params.refine = " in line


# ---- the C++ façade ----

def test_the_facade_methods_compile_against_the_c_abi_alone(fg, tmp_path):
    """include/fgoicp/*.hpp with the robust methods builds with a plain C++17 compiler, warnings as errors; the host half runs without a device"""
    fg.build.build()
    lib_dir = os.path.join(REPO, "fast-go-icp_amd", "lib")
    exe = str(tmp_path / "robust_facade_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "host_harness", "robust_facade_check.cpp"), "-o", exe, "-L" + lib_dir, "-lfgoicp_amd", "-Wl,-rpath," + lib_dir], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "HOST OK 112 272", (p.returncode, p.stdout, p.stderr)
