"""GPU: refinement inside a batch (fgoicp_batch_opts_refine.refine).  The contract is bytes: a pair's refinement in a batch
is the solo call's result struct, whatever shares its fused launches.  Through the test hook fgoicp_batch_test_refine (the backend's own
tick over contexts made here) against fgoicp_icp_plane / _gicp / _robust on the same context and pose; through FastGoICPBatch against
FastGoICP.refine_*; through the command-line tool, lone runs against --batch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
BOX = (1.0, 0.8, 0.6)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SHARED = {}


def _rot(axis, deg):
    a = np.asarray(axis, f64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def _case(fg, nt, ns, seed, **kw):
    """a pre-processed pair, its true pose in that frame and a start 2 - 3 degrees and 0.01 off it"""
    tgt, src, R_gt, t_gt = fg.synth.make_pair(nt, ns, BOX, seed=seed, overlap=1.0, noise=1e-3, angle_deg=20.0, **kw)
    pct, pcs, off_t, off_s, scale, bounds = fg.synth.preprocess(tgt, src)
    t = f64(scale) * (t_gt + off_t.astype(f64) - R_gt @ off_s.astype(f64))
    rng = np.random.default_rng(seed)
    R0 = (_rot(rng.normal(size=3), float(rng.uniform(2.0, 3.0))) @ R_gt).astype(f32)
    t0 = (t + 0.01 * rng.normal(size=3) / np.sqrt(3)).astype(f32)
    return dict(pct=pct, pcs=pcs, bounds=bounds, R0=R0, t0=t0)


def _ctx(fg, c, flags=0, inliers=0, normals_from=None):
    reg = fg.Registration(c["pct"], c["pcs"], c["bounds"], 0.05, flags=flags)
    if inliers:
        reg.set_inliers(inliers)
    if normals_from is None:
        reg.set_target_normals(k=16)
        reg.set_source_normals(k=16)
    else:  # a brute-force context estimates none: another context's
        reg.set_target_normals(normals_from.target_normals())
        reg.set_source_normals(normals_from.source_normals())
    return reg


def _sized(fg):
    """contexts at ns = 40 (one partial block), 255, 256, 257, 513 and 700, nt 600 .. 2500; made once"""
    if "sized" not in _SHARED:
        sizes = ((600, 40), (900, 255), (1300, 256), (1700, 257), (2100, 513), (2500, 700))
        cases = [_case(fg, nt, ns, 4100 + ns) for nt, ns in sizes]
        _SHARED["sized"] = (cases, [_ctx(fg, c) for c in cases])
    return _SHARED["sized"]


class Run:
    """one run of the hook: context frame, max_dist2 and the scale given directly"""

    def __init__(self, model="plane", loss=None, scale=None, max_iter=30, conv_thr=1e-6, max_dist2=np.inf, epsilon=1e-3, start_pass=0):
        self.model, self.loss, self.scale, self.max_iter, self.conv_thr, self.max_dist2, self.epsilon, self.start_pass = model, loss, scale, max_iter, conv_thr, max_dist2, epsilon, start_pass

    def solo(self, reg, R, t):
        call = reg.icp_gicp if self.model == "gicp" else reg.icp_plane
        kw = dict(epsilon=self.epsilon) if self.model == "gicp" else {}
        return call(R, t, max_iter=self.max_iter, conv_thr=self.conv_thr, max_dist2=self.max_dist2, loss=self.loss, loss_scale=self.scale, **kw)


def hook(fg, regs, runs, poses):
    """-> (per run: the result slot's bytes, status, message), fused launches"""
    from fgoicp_amd.nodes import to_glm
    lib = fg._lib.load()
    n = len(regs)
    ctxs = (C.c_void_p * n)(*[r._h.value for r in regs])
    specs = (fg._lib.BatchRefine * n)()
    for s, r in zip(specs, runs):
        s.struct_size = C.sizeof(fg._lib.BatchRefine)
        s.model = fg._lib.MODEL_GICP if r.model == "gicp" else fg._lib.MODEL_PLANE
        s.k, s.max_iter, s.conv_thr, s.max_distance, s.epsilon = 0, r.max_iter, r.conv_thr, r.max_dist2, r.epsilon
        s.loss = fg._lib.LOSS_NONE if r.loss is None else fg._lib.LOSSES[r.loss]
        s.loss_scale = 0.0 if r.scale is None else r.scale
    passes = np.array([r.start_pass for r in runs], np.int32)
    R0 = np.concatenate([to_glm(R) for R, _ in poses]).astype(f32)
    t0 = np.concatenate([np.asarray(t, f32) for _, t in poses]).astype(f32)
    out = (fg._lib.RobustResult * n)()
    status = np.full(n, -1, np.int32)
    msg = C.create_string_buffer(256 * n)
    launches = C.c_uint64(0)
    rc = lib.fgoicp_batch_test_refine(ctxs, n, specs, passes.ctypes.data_as(fg._lib.c_int_p), R0.ctypes.data_as(fg._lib.c_float_p), t0.ctypes.data_as(fg._lib.c_float_p),
                                      out, status.ctypes.data_as(fg._lib.c_int_p), msg, C.byref(launches))
    assert rc == 0, lib.fgoicp_last_error()
    size = C.sizeof(fg._lib.RobustResult)
    raw = bytes(out)
    return [(raw[i * size:(i + 1) * size], int(status[i]), msg.raw[256 * i:256 * (i + 1)].split(b"\0")[0].decode()) for i in range(n)], launches.value


def assert_slot_is_solo(fg, slot, run, solo, what):
    raw, status, msg = slot
    assert status == 0, (what, status, msg)
    if run.loss is None:  # the plain struct in the slot's first bytes, zeros behind it
        n = C.sizeof(fg._lib.PlaneResult)
        assert raw[:n] == solo.raw and not any(raw[n:]), what
    else:
        assert raw == solo.raw, what


def test_hook_mixed_classes_and_staggered_starts_return_the_solo_bytes(fg, gpu_required):
    """all four classes in one call — plane, GICP, plane + Tukey with an estimated scale, GICP + Huber with a given one — over every block
    shape, the runs starting at passes 0, 0, 1, 3, 0, 1"""
    cases, regs = _sized(fg)
    runs = [Run("plane", start_pass=0), Run("gicp", start_pass=0), Run("plane", "tukey", None, start_pass=1), Run("gicp", "huber", 0.01, start_pass=3),
            Run("gicp", "tukey", None, start_pass=0), Run("plane", start_pass=1)]
    poses = [(c["R0"], c["t0"]) for c in cases]
    solo = [r.solo(reg, *p) for r, reg, p in zip(runs, regs, poses)]
    assert all(s.iterations >= 1 and s.correspondences > 0 for s in solo), [(s.iterations, s.correspondences) for s in solo]
    got, launches = hook(fg, regs, runs, poses)
    for i, (slot, run, s) in enumerate(zip(got, runs, solo)):
        assert_slot_is_solo(fg, slot, run, s, i)
    again, launches2 = hook(fg, regs, runs, poses)
    assert [g[0] for g in again] == [g[0] for g in got] and launches2 == launches
    # the classes the other way round over the same contexts: other block shapes per class, other company per launch
    runs2 = runs[::-1]
    solo2 = [r.solo(reg, *p) for r, reg, p in zip(runs2, regs, poses)]
    got2, _ = hook(fg, regs, runs2, poses)
    for i, (slot, run, s) in enumerate(zip(got2, runs2, solo2)):
        assert_slot_is_solo(fg, slot, run, s, ("reversed", i))


def test_hook_edges(fg, gpu_required):
    cases, regs = _sized(fg)
    c = cases[5]
    trimmed = _ctx(fg, c, flags=fg.FLAG_CURVE_ORDER, inliers=int(0.8 * len(c["pcs"])))
    brute = _ctx(fg, cases[4], flags=fg.FLAG_BRUTE_FORCE_NN, normals_from=regs[4])
    # a source that is an exact subset of the target, at the identity: every residual is 0, there is no scale to estimate
    sub = dict(cases[3])
    sub["pcs"] = np.ascontiguousarray(sub["pct"][::7][:200])
    subset = _ctx(fg, sub)
    I, z = np.eye(3, dtype=f32), np.zeros(3, f32)
    use = [regs[0], regs[1], regs[2], trimmed, brute, subset, regs[5]]
    runs = [Run("plane", max_iter=0), Run("gicp", max_dist2=0.0), Run("plane", "tukey", 1e-12), Run("plane", "cauchy", None, start_pass=1), Run("gicp", "geman_mcclure", 0.02),
            Run("plane", "huber", None), Run("gicp", start_pass=2)]
    poses = [(cases[0]["R0"], cases[0]["t0"]), (cases[1]["R0"], cases[1]["t0"]), (cases[2]["R0"], cases[2]["t0"]), (c["R0"], c["t0"]), (cases[4]["R0"], cases[4]["t0"]), (I, z),
             (c["R0"], c["t0"])]
    solo = []
    for r, reg, p in zip(runs, use, poses):
        try:
            solo.append(r.solo(reg, *p))
        except fg.FgoicpError as e:
            solo.append(e)
    assert solo[0].iterations == 0 and solo[0].correspondences > 0                       # max_iter = 0: the start, evaluated
    assert solo[1].iterations == 0 and solo[1].correspondences == 0                      # nothing counted: one evaluation
    assert solo[2].iterations == 0 and solo[2].weight_sum == 0.0 and solo[2].correspondences > 0  # a Tukey scale below every residual
    assert solo[3].iterations >= 1 and solo[4].iterations >= 1 and solo[6].iterations >= 1
    assert isinstance(solo[5], fg.FgoicpError) and "the median residual is 0" in str(solo[5]) and "pass a scale" in str(solo[5])
    got, _ = hook(fg, use, runs, poses)
    for i, (slot, run, s) in enumerate(zip(got, runs, solo)):
        if i == 5:  # that run's own refusal, with the solo call's status and message; its slot stays zero
            assert slot[1] == s.status == 1 and slot[2] and slot[2] in str(s) and slot[2].startswith("fgoicp_icp_robust") and not any(slot[0]), slot[1:]
        else:
            assert_slot_is_solo(fg, slot, run, s, i)
    # normals not set: that run's refusal with the solo call's message, the other run untouched
    bare = fg.Registration(cases[1]["pct"], cases[1]["pcs"], cases[1]["bounds"], 0.05)
    with pytest.raises(fg.FgoicpError) as e:
        bare.icp_plane(cases[1]["R0"], cases[1]["t0"])
    got, _ = hook(fg, [bare, regs[0]], [Run("plane"), Run("plane")], [(cases[1]["R0"], cases[1]["t0"]), (cases[0]["R0"], cases[0]["t0"])])
    assert got[0][1] == 1 and "the target normals are not set" in got[0][2] and got[0][2] in str(e.value)
    assert_slot_is_solo(fg, got[1], Run("plane"), Run("plane").solo(regs[0], cases[0]["R0"], cases[0]["t0"]), "next to a refused run")
    for r in (trimmed, brute, subset, bare):
        r.close()


@pytest.mark.parametrize("model,loss", [("plane", None), ("gicp", "cauchy")], ids=["plane", "gicp-cauchy"])
def test_hook_one_class_makes_one_fused_launch_per_tick(fg, gpu_required, model, loss):
    """n runs of one class from pass 0: every loop makes iterations + 1 evaluations, one per tick, and a tick of one class is one fused
    launch — so the launches are max(iterations) + 1: a condition, not a measurement"""
    cases, regs = _sized(fg)
    runs = [Run(model, loss, None if loss is None else 0.02, max_iter=3 + 4 * i) for i in range(len(regs))]
    poses = [(c["R0"], c["t0"]) for c in cases]
    got, launches = hook(fg, regs, runs, poses)
    solo = [r.solo(reg, *p) for r, reg, p in zip(runs, regs, poses)]
    for i, (slot, run, s) in enumerate(zip(got, runs, solo)):
        assert_slot_is_solo(fg, slot, run, s, i)
    iters = [s.iterations for s in solo]
    assert len(set(iters)) > 1, iters  # loops of different lengths share the ticks
    assert launches == max(iters) + 1, (launches, iters)


# ---- the whole batch ----------------------------------------------------------------------------------------------------------------
SPECS = [None, {"model": "plane"}, {"model": "gicp"}, {"model": "plane", "loss": "cauchy"}, {"model": "gicp", "loss": "tukey"}, {"model": "plane", "max_distance": 0.05}]


def _batch_pairs(fg):
    if "pairs" not in _SHARED:
        rng = np.random.default_rng(11)
        pairs = []
        for i in range(6):
            ns = int(rng.integers(500, 1501))
            nt = int(rng.integers(max(1000, ns), 3001))
            tgt, src, _, _ = fg.synth.make_pair(nt, ns, BOX, seed=5200 + i, angle_deg=float(rng.uniform(10, 40)), outlier_frac=0.05 if i in (3, 4) else 0.0)
            pairs.append((tgt, src, 0.05, (1e-3, 2e-3)[i % 2]))
        solo = []
        for (tgt, src, lut, mse), spec in zip(pairs, SPECS):
            s = fg.FastGoICP(tgt, src, lut, mse, schedule=1, round_width=0)
            s.run()
            ref = None
            if spec is not None:
                kw = {k: v for k, v in spec.items() if k != "model"}
                ref = (s.refine_gicp if spec["model"] == "gicp" else s.refine_plane)(**kw)
            solo.append(ref)
            s.close()
        plain = fg.FastGoICPBatch(pairs, schedule=1, round_width=0, alignment=True, information=True)
        out = plain.run()
        base = [(out[i], plain.get_best_error(i), plain.stats(i), plain.alignment(i), plain.information(i)) for i in range(6)]
        plain.close()
        _SHARED["pairs"] = (pairs, solo, base)
    return _SHARED["pairs"]


def _same_arrays(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("max_live,perm", [(1, None), (3, None), (0, None), (3, [4, 1, 5, 0, 3, 2])], ids=["live1", "live3", "auto", "permuted"])
def test_whole_batch_refines_as_the_solo_solvers_and_leaves_the_search_alone(fg, gpu_required, max_live, perm):
    pairs, solo, base = _batch_pairs(fg)
    order = perm or list(range(6))
    b = fg.FastGoICPBatch([pairs[i] for i in order], schedule=1, round_width=0, max_live=max_live, alignment=True, information=True, refine=[SPECS[i] for i in order])
    out = b.run()
    for k, i in enumerate(order):
        (R, t), err, st, al, inf = base[i]
        assert out[k] is not None and _same_arrays(out[k][0], R) and _same_arrays(out[k][1], t), k
        assert f32(b.get_best_error(k)).tobytes() == f32(err).tobytes(), k
        sb = b.stats(k)
        assert all(sb[key] == st[key] for key in ("trans_cubes", "rot_cubes", "inner_bnb", "icp_runs", "icp_iters", "rounds", "initial_icp_sse")), k
        a2, i2 = b.alignment(k), b.information(k)
        assert all(_same_arrays(getattr(a2, f), getattr(al, f)) for f in ("indices", "dist2", "inlier", "target_hit")) and (a2.points, a2.inliers, a2.targets_hit, a2.sse.tobytes(), a2.max_inlier_dist2.tobytes(), a2.scaling_factor.tobytes()) == (
            al.points, al.inliers, al.targets_hit, al.sse.tobytes(), al.max_inlier_dist2.tobytes(), al.scaling_factor.tobytes()), k
        assert i2.raw == inf.raw, k
        if solo[i] is None:
            with pytest.raises(fg.FgoicpError, match="has no refinement"):
                b.refined(k)
            with pytest.raises(fg.FgoicpError, match="has no refinement"):
                b.refined_information(k)
            continue
        r = b.refined(k)
        assert type(r) is type(solo[i]) and r.raw == solo[i].raw, (k, i, r.iterations, solo[i].iterations)
        assert r.iterations >= 1 and r.rank == 6
        ri = b.refined_information(k)
        assert ri.correspondences > 0 and ri.raw != i2.raw  # the refined pose's, not the search's
    launches, evals = b.refine_launches()
    want = sum(s.iterations + 1 for s in solo if s is not None)
    assert evals == want and 0 < launches <= evals, (launches, evals, want)
    b.close()


def test_a_refused_refinement_leaves_its_pair_and_the_others_alone(fg, gpu_required):
    """a distance threshold below every distance and a loss without a scale: nothing is counted at the search's pose and the scale estimate
    refuses — the pair keeps its search result and status, the getter returns the refinement's own status and message"""
    pairs, solo, base = _batch_pairs(fg)
    spec = {"model": "plane", "loss": "huber", "max_distance": 1e-9}
    b = fg.FastGoICPBatch([pairs[1], pairs[3], pairs[2]], schedule=1, round_width=0, refine=[SPECS[1], spec, SPECS[2]])
    out = b.run()
    assert all(o is not None for o in out) and [b.status(i) for i in range(3)] == [0, 0, 0]
    for k, i in enumerate((1, 3, 2)):
        (R, t), err = base[i][0], base[i][1]
        assert _same_arrays(out[k][0], R) and _same_arrays(out[k][1], t) and f32(b.get_best_error(k)).tobytes() == f32(err).tobytes(), k
    assert b.refined(0).raw == solo[1].raw and b.refined(2).raw == solo[2].raw
    s = fg.FastGoICP(*pairs[3], schedule=1, round_width=0)
    s.run()
    with pytest.raises(fg.FgoicpError) as want:
        s.refine_plane(loss="huber", max_distance=1e-9)
    s.close()
    with pytest.raises(fg.FgoicpError) as got:
        b.refined(1)
    assert got.value.status == want.value.status == 1
    tail = str(want.value).split(": ", 1)[1]
    assert "pass a scale" in tail and tail in str(got.value), (str(got.value), str(want.value))
    b.close()


# ---- the command-line tool ----------------------------------------------------------------------------------------------------------
def _write_txt(path, pts):
    with open(path, "w") as f:
        f.write(f"{len(pts)}\n")
        for p in pts:
            f.write(f"{p[0]:.9g} {p[1]:.9g} {p[2]:.9g}\n")


def test_cli_batch_refines_every_config_as_a_lone_run_does(fg, gpu_required, tmp_path):
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    extras = {"a": 'refine = "plane"\nrefine_loss = "huber"\n', "b": 'refine = "gicp"\nrefine_knn = 12\ninformation_distance = 0.05\n'}
    for j, tag in enumerate(extras):
        tgt, src, _, _ = fg.synth.make_pair(1500, 600, BOX, seed=5300 + j, angle_deg=25.0, outlier_frac=0.05)
        _write_txt(tmp_path / f"{tag}_tgt.txt", tgt)
        _write_txt(tmp_path / f"{tag}_src.txt", src)
    def config(tag, kind):
        info = f'information = "{tmp_path}/{tag}_{kind}_info.txt"\n' if tag == "b" else ""
        (tmp_path / f"{tag}_{kind}.toml").write_text(f'[io]\ntarget = "{tmp_path}/{tag}_tgt.txt"\nsource = "{tmp_path}/{tag}_src.txt"\noutput = "{tmp_path}/{tag}_{kind}_out.toml"\n{info}'
                                                     f'[params]\nlut_resolution = 0.05\nmse_threshold = 0.001\nseed = 3\n{extras[tag]}')
    logs = {}
    for tag in extras:
        config(tag, "lone")
        config(tag, "batch")
        p = subprocess.run([exe, "-c", str(tmp_path / f"{tag}_lone.toml")], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        logs[tag] = [ln for ln in (p.stdout + p.stderr).splitlines() if "refinement:" in ln]
        assert len(logs[tag]) == 1
    (tmp_path / "list.txt").write_text("a_batch.toml\nb_batch.toml\n")
    p = subprocess.run([exe, "--batch", str(tmp_path / "list.txt")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    blog = [ln for ln in (p.stdout + p.stderr).splitlines() if "refinement:" in ln]
    assert len(blog) == 2
    lines = lambda name: [ln for ln in (tmp_path / name).read_text().splitlines() if not ln.startswith("seconds")]
    for j, tag in enumerate(extras):
        lone, batch = lines(f"{tag}_lone_out.toml"), lines(f"{tag}_batch_out.toml")
        assert "[refined]" in lone and lone == batch, (tag, lone, batch)
        # the lone run's refinement line, behind the batch's per-pair prefix
        text = re.search(r"(Point-to-plane|Generalized-ICP) refinement:.*$", logs[tag][0]).group(0)
        assert any(ln.endswith(f"Pair {j}: {text}") for ln in blog), (text, blog)
    assert (tmp_path / "b_lone_info.txt").read_bytes() == (tmp_path / "b_batch_info.txt").read_bytes()
    assert "huber loss" in logs["a"][0] and "epsilon" in logs["b"][0]
