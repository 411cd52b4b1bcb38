"""GPU: the information matrix of a registration — the moments of the counted correspondences from the device (align_info_kernel,
moment_fold_kernel of csrc/device/fixed_sum.hpp) against numpy on the alignment report, for a context (fgoicp_information), a solver (fgoicp_solver_information),
a batch (fgoicp_batch_information), the CLI (io.information) and the C++ facade."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import np_restatement as npr

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
EPS = 2.0 ** -52
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # xx xy xz yy yz zz


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def counted(a, nt, max_dist2=np.inf):
    return a.inlier & (a.dist2 <= f32(max_dist2)) & (a.indices < nt)


def check_against_report(info, a, tgt, max_dist2=np.inf):
    """the moments recomputed in float64 from the report and the target as passed in: the count equal, every moment within
    N 2^-52 sum |term| (the products are exact in fp64, only the order of the additions differs), the matrix the moments' matrix"""
    m = counted(a, len(tgt), max_dist2)
    n = int(m.sum())
    assert info.correspondences == n and info.points == len(a.indices)
    q = tgt[a.indices[m]].astype(f64)
    terms = [q[:, 0], q[:, 1], q[:, 2]] + [q[:, i] * q[:, j] for i, j in PAIRS] + [a.dist2[m].astype(f64)]
    got = list(info.sum_q) + list(info.sum_qq) + [info.sum_dist2]
    for k, (t, g) in enumerate(zip(terms, got)):
        tol = n * EPS * float(np.abs(t).sum())
        assert abs(float(t.sum()) - g) <= tol, (k, float(t.sum()), g, tol)
    xx, xy, xz, yy, yz, zz = info.sum_qq
    x, y, z = info.sum_q
    want = np.array([[yy + zz, -xy, -xz, 0, -z, y], [-xy, xx + zz, -yz, z, 0, -x], [-xz, -yz, xx + yy, -y, x, 0],
                     [0, z, -y, n, 0, 0], [-z, 0, x, 0, n, 0], [y, -x, 0, 0, 0, n]], f64)
    assert np.array_equal(info.matrix, want + 0.0)
    assert info.fitness == n / len(a.indices)
    assert info.inlier_rmse == pytest.approx(np.sqrt(a.dist2[m].astype(f64).mean()) / float(info.scaling_factor) if n else 0.0, rel=1e-9)
    return n


def check_bits_against_report(info, a, tgt, max_dist2=np.inf):
    """the ten sums restated in the device's fixed order (oracle/np_restatement.py fixed_order_sum) over terms formed in float64 from the
    report and the target — a product of two floats is exact in a double; an index that is not counted contributes a row of +0.0: every bit"""
    m = counted(a, len(tgt), max_dist2)
    q = tgt[np.where(m, a.indices, 0)].astype(f64)
    terms = np.column_stack([q[:, 0], q[:, 1], q[:, 2]] + [q[:, i] * q[:, j] for i, j in PAIRS] + [a.dist2.astype(f64)])
    terms[~m] = 0.0
    want = npr.fixed_order_sum(terms)
    got = np.array(list(info.sum_q) + list(info.sum_qq) + [info.sum_dist2], f64)
    assert info.correspondences == int(m.sum())
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got - want, int(m.sum()))


def _clouds(ns, nt, seed):
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(-1, 1, (nt, 3)).astype(f32)
    src = rng.uniform(-0.9, 0.9, (ns, 3)).astype(f32)
    return tgt, src, np.array([[-1, 1]] * 3, f32)


def _transform(fg, seed):
    from fgoicp_amd.synth import random_rotation
    rng = np.random.default_rng(seed)
    return random_rotation(rng, 40.0).astype(f32), rng.uniform(-0.1, 0.1, 3).astype(f32)


# ---- 1. against the report ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,nt", [(1, 500), (63, 500), (64, 500), (257, 17), (1000, 500)])
def test_moments_are_the_reports_moments(fg, gpu_required, ns, nt):
    """ns: a partial wave, a full wave, a partial block, several blocks; nt = 17 once.  Contexts: default, caller order, brute force, and
    trimmed with the cut inside a group of equal distances (duplicated source points: the report's tie rule decides who is counted)."""
    tgt, src, bounds = _clouds(ns, nt, 100 + ns)
    R, t = _transform(fg, ns)
    dup = [j for j in (0, 5, 11, 40, 62) if j < ns]
    src[dup] = src[0]
    ref = None
    for flags in (0, fg.FLAG_NO_MORTON, fg.FLAG_BRUTE_FORCE_NN):
        reg = fg.Registration(tgt, src, bounds, 0.1, flags=flags)
        a, info = reg.alignment(R, t), reg.information(R, t)
        assert check_against_report(info, a, tgt) == ns and info.scaling_factor == 1.0 and np.isinf(info.max_dist2)
        # the report's arrays do not depend on the context's order or search, and the sums' order is fixed by the caller index: the same bytes
        ref = ref or info.raw
        assert info.raw == ref
        reg.close()
    if ns < 8:
        return
    below = int((a.dist2 < a.dist2[0]).sum())
    k = below + 2  # two of the five tied points are inliers: those with the lowest caller indices
    reg = fg.Registration(tgt, src, bounds, 0.1, flags=fg.FLAG_CURVE_ORDER)
    reg.set_inliers(k)
    a, info = reg.alignment(R, t), reg.information(R, t)
    assert a.inliers == k and list(a.inlier[dup]) == [True, True] + [False] * (len(dup) - 2) and len(set(_bits(a.dist2[dup]))) == 1
    assert check_against_report(info, a, tgt) == k
    thr = a.dist2[0]  # a threshold at the tied distance keeps the tie rule's choice, one below it drops the group
    assert check_against_report(reg.information(R, t, thr), a, tgt, thr) == k
    lower = np.nextafter(thr, f32(0))
    assert check_against_report(reg.information(R, t, lower), a, tgt, lower) == below
    reg.close()


@pytest.mark.parametrize("trimmed", [False, True], ids=["untrimmed", "trimmed"])
@pytest.mark.parametrize("ns", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_sums_have_the_bits_of_the_fixed_order(fg, gpu_required, ns, trimmed):
    """ns: a partial wave, a full wave and one lane more, a block less one lane, a block, a block and one lane, four blocks; trimmed at
    0.8 ns (uncounted lanes among the counted), and with a threshold at the median distance"""
    tgt, src, bounds = _clouds(ns, 500, 300 + ns)
    R, t = _transform(fg, ns)
    reg = fg.Registration(tgt, src, bounds, 0.1, flags=fg.FLAG_CURVE_ORDER if trimmed else 0)
    if trimmed:
        reg.set_inliers(max(1, int(0.8 * ns)))
    a = reg.alignment(R, t)
    assert a.inliers == (max(1, int(0.8 * ns)) if trimmed else ns)
    check_bits_against_report(reg.information(R, t), a, tgt)
    med = np.sort(a.dist2)[ns // 2]
    check_bits_against_report(reg.information(R, t, med), a, tgt, med)
    reg.close()


# ---- 2. the threshold ---------------------------------------------------------------------------------------------------------------
def test_threshold_counts_the_entries_at_or_below_it(fg, gpu_required):
    tgt, src, bounds = _clouds(1000, 500, 7)
    R, t = _transform(fg, 7)
    reg = fg.Registration(tgt, src, bounds, 0.1)
    a = reg.alignment(R, t)
    assert check_against_report(reg.information(R, t, np.inf), a, tgt) == a.inliers == 1000
    assert reg.information(R, t).raw == reg.information(R, t, np.inf).raw
    med = np.sort(a.dist2)[500]  # an entry of dist2: `<=` counts it
    n = check_against_report(reg.information(R, t, med), a, tgt, med)
    assert n == int((a.dist2 <= med).sum()) >= 501
    assert a.dist2.min() > 0  # no exact hits
    zero = reg.information(R, t, 0.0)
    assert zero.correspondences == 0 and not zero.matrix.any() and not np.signbit(zero.matrix).any() and zero.sum_dist2 == 0 and zero.inlier_rmse == 0
    for bad in (float("nan"), -1.0, -np.inf):
        with pytest.raises(fg.FgoicpError) as e:
            reg.information(R, t, bad)
        assert e.value.status == 1 and "max_dist2" in str(e.value)
    # a caller's shorter struct is not overrun: 64 of the 400 bytes are written, and they are the first 64 of the whole answer
    lib = fg._lib.load()
    buf = (C.c_ubyte * 512)(*([0xA5] * 512))
    out = C.cast(buf, C.POINTER(fg._lib.Information))
    out.contents.struct_size = 64
    from fgoicp_amd.nodes import to_glm
    fp = fg._lib.c_float_p
    assert lib.fgoicp_information(reg._h, to_glm(R).ctypes.data_as(fp), t.ctypes.data_as(fp), float(med), out) == 0
    whole = reg.information(R, t, med).raw
    assert bytes(buf)[64:] == bytes([0xA5] * 448) and bytes(buf)[4:64] == whole[4:64] and out.contents.struct_size == 64
    out.contents.struct_size = 0
    assert lib.fgoicp_information(reg._h, to_glm(R).ctypes.data_as(fp), t.ctypes.data_as(fp), float(med), out) == 1
    reg.close()


# ---- 3. the fold's strided loop -----------------------------------------------------------------------------------------------------
def test_more_than_1024_partial_rows(fg, gpu_required):
    """270 000 source points: 1055 blocks, so thread t of the fold adds rows t and t + 1024; the sums bit for bit in the fixed order"""
    tgt, src, R_gt, _ = fg.synth.make_pair(40000, 270000, (1.0, 0.8, 0.6), seed=77, angle_deg=20.0, outlier_frac=0.0)
    pct, pcs, *_, bounds = fg.synth.preprocess(tgt, src)
    reg = fg.Registration(pct, pcs, bounds, 0.05)
    R, t = R_gt.astype(f32), np.zeros(3, f32)
    a = reg.alignment(R, t)
    info = reg.information(R, t)
    assert check_against_report(info, a, pct) == 270000
    check_bits_against_report(info, a, pct)
    thr = np.sort(a.dist2)[100000]
    near = reg.information(R, t, thr)
    check_against_report(near, a, pct, thr)
    check_bits_against_report(near, a, pct, thr)
    reg.close()


# ---- 4. reproducible and harmless ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trimmed", [False, True], ids=["untrimmed", "trimmed"])
def test_two_calls_are_the_same_bytes_and_the_context_is_left_as_found(fg, gpu_required, trimmed):
    tgt, src, _, _ = fg.synth.make_pair(3000, 1500, (1.0, 0.8, 0.6), seed=31, angle_deg=30.0, outlier_frac=0.1 if trimmed else 0.0)
    pct, pcs, *_, bounds = fg.synth.preprocess(tgt, src)
    R, t = _transform(fg, 31)

    def others(reg):
        e, Ri, ti = fg.IterativeClosestPoint3D(reg, max_iter=20, convergence_threshold=0.005, R=R, t=t).run()
        a = reg.alignment(R, t)
        return [_bits(reg.compute_sse_error(R, t)), _bits(e), _bits(Ri), _bits(ti), a.indices, _bits(a.dist2), a.inlier, a.target_hit, _bits(a.sse)]

    reg = fg.Registration(pct, pcs, bounds, 0.05, flags=fg.FLAG_CURVE_ORDER if trimmed else 0)
    if trimmed:
        reg.set_inliers(1200)
    before = others(reg)
    thr = np.sort(before[5].view(f32))[500]  # a third of the points lie within it
    one = reg.information(R, t, thr)
    two = reg.information(R, t, thr)
    assert one.raw == two.raw and 0 < one.correspondences < (1200 if trimmed else 1500)
    after = others(reg)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    assert reg.information(R, t, thr).raw == one.raw  # ... and behind an ICP and a report
    reg.close()


# ---- 5. the solver ------------------------------------------------------------------------------------------------------------------
def _pairs(fg, seed=0):
    """(tgt, src, lut, mse, trim): small pairs, one of them trimmed, large rotations so that the search runs"""
    rng = np.random.default_rng(seed)
    out = []
    for i, frac in enumerate((0.0, 0.2, 0.0, 0.0)):
        tgt, src, _, _ = fg.synth.make_pair(int(rng.integers(1500, 3001)), int(rng.integers(400, 1201)), (1.0, 0.8, 0.6), seed=700 + 7 * seed + i, angle_deg=150.0,
                                            min_angle_deg=100.0, outlier_frac=0.05 if frac else 0.0)
        out.append((tgt + f32(3.0 * i), src, (0.05, 0.04)[i % 2], (1e-3, 5e-4)[i % 2], frac))  # targets off the origin: the change of frame has work to do
    return out


def direct_information(q):
    info = np.zeros((6, 6))
    for x, y, z in np.asarray(q, f64):
        G = np.array([[0.0, z, -y, 1, 0, 0], [-z, 0.0, x, 0, 1, 0], [y, -x, 0.0, 0, 0, 1]])
        info += G.T @ G
    return info


@pytest.mark.parametrize("schedule,round_width", [(0, 1), (1, 0)], ids=["serial", "round"])
def test_solver_information_in_the_callers_frame(fg, gpu_required, schedule, round_width):
    for tgt, src, lut, mse, frac in _pairs(fg, seed=5)[:2]:
        s = fg.FastGoICP(tgt, src, lut, mse, schedule=schedule, round_width=round_width, trim_fraction=frac)
        with pytest.raises(fg.FgoicpError) as e:  # before run(): refused
            s.information()
        assert e.value.status == 1 and "has not succeeded" in str(e.value)
        R1, t1 = s.run()
        e1 = s.get_best_error()
        info, a, pre = s.information(), s.alignment(), s.preproc()
        assert info.correspondences == a.inliers and _bits(info.scaling_factor) == _bits(pre["scale"]) and info.fitness == a.fitness
        assert info.inlier_rmse == pytest.approx(a.inlier_rmse, rel=1e-6)
        # the same code path by hand: the context's moments at the best transform through fgoicp_information_from_moments
        Rb, tb = s.get_best_transform()
        ctx = s.registration.information(Rb, tb)
        m, q, qq = fg.information_from_moments(ctx.correspondences, ctx.sum_q, ctx.sum_qq, offset=-pre["offset_pct"], scale=pre["scale"])  # the offset is minus the centroid
        assert np.array_equal(m.view(np.uint64), info.matrix.view(np.uint64)) and np.array_equal(q, info.sum_q) and np.array_equal(qq, info.sum_qq)
        assert ctx.sum_dist2 == info.sum_dist2
        # numpy on the ORIGINAL target points and the report's correspondences: the normalised coordinates carry two fp32 roundings each
        # and the matrix is quadratic in them
        qo = tgt[a.indices[a.inlier]]
        tol = 16 * 2.0 ** -24 * len(qo) * float(np.abs(qo.astype(f64)).max()) ** 2
        dev = np.abs(info.matrix - direct_information(qo)).max()
        print(f"schedule {schedule} trim {frac}: largest deviation from numpy on the raw target {dev:.4g}, tolerance {tol:.4g}")
        assert dev <= tol
        # a distance in the callers' units counts exactly dist2 <= (float32(d) * scale)^2, evaluated in float32
        d = float(np.median(a.distances[a.inlier]))
        ds = f32(f32(d) * pre["scale"])
        thr = f32(ds * ds)
        near = s.information(d)
        assert _bits(near.max_dist2) == _bits(thr)
        assert near.correspondences == int(counted(a, len(tgt), thr).sum()) and 0 < near.correspondences < a.inliers
        qn = tgt[a.indices[counted(a, len(tgt), thr)]]
        assert np.abs(near.matrix - direct_information(qn)).max() <= tol
        # a second run returns the same bits, and so does the call after it
        R2, t2 = s.run()
        assert np.array_equal(_bits(R1), _bits(R2)) and np.array_equal(_bits(t1), _bits(t2)) and _bits(e1) == _bits(s.get_best_error())
        assert s.information().raw == info.raw and s.information(d).raw == near.raw
        for bad in (float("nan"), -0.5):
            with pytest.raises(fg.FgoicpError):
                s.information(bad)
        s.close()


# ---- 6. the batch -------------------------------------------------------------------------------------------------------------------
def _same_alignment(a, b):
    assert np.array_equal(a.indices, b.indices) and np.array_equal(_bits(a.dist2), _bits(b.dist2)) and np.array_equal(a.inlier, b.inlier)
    assert np.array_equal(a.target_hit, b.target_hit) and (a.points, a.inliers, a.targets_hit) == (b.points, b.inliers, b.targets_hit)
    assert _bits(a.sse) == _bits(b.sse) and _bits(a.max_inlier_dist2) == _bits(b.max_inlier_dist2) and _bits(a.scaling_factor) == _bits(b.scaling_factor)


@pytest.mark.parametrize("schedule,round_width", [(0, 1), (1, 0)], ids=["serial", "round"])
def test_batch_information_is_the_solo_solvers(fg, gpu_required, schedule, round_width):
    pairs = _pairs(fg, seed=6)
    dist = None
    solo = []
    for tgt, src, lut, mse, frac in pairs:
        s = fg.FastGoICP(tgt, src, lut, mse, schedule=schedule, round_width=round_width, trim_fraction=frac)
        s.run()
        a = s.alignment()
        if dist is None:
            dist = float(np.median(a.distances))  # the batch's one threshold: half of the first pair's points lie within it
        solo.append((s.information(), s.information(dist), a))
        s.close()
    assert all(0 < near.correspondences for _, near, _ in solo) and solo[0][1].correspondences < solo[0][0].correspondences
    for max_live in (1, 0):
        for alignment in (True, False):
            for information, which in ((True, 0), (dist, 1)):
                if information is True and max_live == 0:
                    continue  # the option without a distance once per alignment setting
                b = fg.FastGoICPBatch(pairs, schedule=schedule, round_width=round_width, max_live=max_live, alignment=alignment, information=information)
                with pytest.raises(fg.FgoicpError):
                    b.information(0)  # before run()
                out = b.run()
                for i in range(len(pairs)):
                    assert out[i] is not None
                    assert b.information(i).raw == solo[i][which].raw, (max_live, alignment, information, i)
                    if alignment:
                        _same_alignment(b.alignment(i), solo[i][2])  # unchanged by the new option
                b.close()
    # a pair that failed (LUT dims above 4094) is refused, the others are served; the option off is refused after the run too
    bad = (pairs[0][0], pairs[0][1], 1e-4, 1e-3, 0.0)
    b = fg.FastGoICPBatch([pairs[0], bad], schedule=schedule, round_width=round_width, information=dist)
    out = b.run()
    assert out[1] is None and b.information(0).raw == solo[0][1].raw
    with pytest.raises(fg.FgoicpError) as e:
        b.information(1)
    assert e.value.status == 1 and "failed" in str(e.value)
    b.close()


# ---- 7. the CLI and the C++ facade --------------------------------------------------------------------------------------------------
def _write_txt(path, pts):
    with open(path, "w") as f:
        f.write(f"{len(pts)}\n")
        for x, y, z in pts:
            f.write(f"{x:.9g} {y:.9g} {z:.9g}\n")


def test_cli_writes_the_matrix_the_solver_returns(fg, gpu_required, tmp_path):
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    tgt, src, lut, mse, _ = _pairs(fg, seed=7)[0]
    _write_txt(tmp_path / "tgt.txt", tgt)
    _write_txt(tmp_path / "src.txt", src)
    dist = 0.03
    for tag, extra in (("with", f"information_distance = {dist}\n"), ("plain", "")):
        io = f'alignment = "{tmp_path}/align.txt"\ninformation = "{tmp_path}/info.txt"\n' if tag == "with" else ""
        (tmp_path / f"{tag}.toml").write_text(f'[io]\ntarget = "{tmp_path}/tgt.txt"\nsource = "{tmp_path}/src.txt"\noutput = "{tmp_path}/{tag}_out.toml"\n{io}'
                                              f'[params]\nlut_resolution = {lut}\nmse_threshold = {mse}\nseed = 3\n{extra}')
        p = subprocess.run([exe, "-c", str(tmp_path / f"{tag}.toml")], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    strip = lambda name: [ln for ln in (tmp_path / name).read_text().splitlines() if not ln.startswith("seconds")]
    assert strip("with_out.toml") == strip("plain_out.toml")  # out.toml does not change
    lines = (tmp_path / "info.txt").read_text().splitlines()
    assert len(lines) == 7 and lines[0].startswith("# information: correspondences = ")
    head = {kv.split(" = ")[0]: float(kv.split(" = ")[1]) for kv in lines[0][len("# information: "):].split(", ")}
    # the source as the CLI registered it (after source_subsample) is in the alignment file
    xyz = np.array([[f32(v) for v in ln.split()[:3]] for ln in (tmp_path / "align.txt").read_text().splitlines()[2:]], f32)
    s = fg.FastGoICP(tgt, xyz, lut, mse)
    s.run()
    info = s.information(dist)
    assert np.array_equal(np.loadtxt(tmp_path / "info.txt"), info.matrix)  # precision 17: the doubles themselves
    assert head["correspondences"] == info.correspondences and head["distance"] == pytest.approx(dist, rel=1e-6)
    assert head["fitness"] == pytest.approx(info.fitness, rel=1e-8) and head["inlier_rmse"] == pytest.approx(info.inlier_rmse, rel=1e-8)
    s.close()
    # --batch writes the same file for a config that names one
    (tmp_path / "b.toml").write_text((tmp_path / "with.toml").read_text().replace("info.txt", "binfo.txt").replace("align.txt", "balign.txt"))
    (tmp_path / "list.txt").write_text("b.toml\nplain.toml\n")
    p = subprocess.run([exe, "--batch", str(tmp_path / "list.txt")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert (tmp_path / "binfo.txt").read_text() == (tmp_path / "info.txt").read_text()


def test_cpp_facade_returns_what_python_returns(fg, gpu_required, tmp_path):
    exe = str(tmp_path / "facade_information_check")
    lib_dir = os.path.join(REPO, "fast-go-icp_amd", "lib")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "host_harness", "facade_information_check.cpp"), "-o", exe, "-L" + lib_dir, "-lfgoicp_amd", "-Wl,-rpath," + lib_dir], check=True)
    tgt, src, lut, _, _ = _pairs(fg, seed=8)[0]
    _write_txt(tmp_path / "tgt.txt", tgt)
    _write_txt(tmp_path / "src.txt", src)
    s = fg.FastGoICP(tgt, src, lut, 1e-3)
    s.run()
    for d in (0.0, 0.03):
        p = subprocess.run([exe, str(tmp_path / "tgt.txt"), str(tmp_path / "src.txt"), str(lut), str(d)], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        got = json.loads(p.stdout.strip().splitlines()[-1])
        info = s.information(d if d else None)
        assert (got["points"], got["correspondences"]) == (info.points, info.correspondences)
        assert np.array_equal(np.array(got["matrix"], f64).reshape(6, 6), info.matrix) and got["m00"] == info.matrix[0, 0]
        assert got["fitness"] == info.fitness and got["inlier_rmse"] == pytest.approx(info.inlier_rmse, rel=1e-12)
    s.close()
