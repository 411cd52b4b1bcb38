"""GPU: fgoicp_batch / FastGoICPBatch — many pairs in one run on one device.  Every pair must return the bits of its own
FastGoICP.run() (R, restored t, best error, the search counters), whatever the schedule, the window, the order or the company."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CONTRACT = ("trans_cubes", "rot_cubes", "inner_bnb", "icp_runs", "icp_iters", "rounds", "initial_icp_sse")
ERR_INVALID_ARG = 1


def _pairs(fg, n=16, seed=0):
    """ns 500..6000, nt 1000..20000; LUT resolutions from 0.01 (sparse: apron-bricked quads) to 0.05 (dense: z-pairs)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ns = int(rng.integers(500, 6001))
        nt = int(rng.integers(max(1000, ns), 20001))
        tgt, src, _, _ = fg.synth.make_pair(nt, ns, (1.0, 0.8, 0.6), seed=1000 + 17 * seed + i, angle_deg=float(rng.uniform(10, 60)))
        lut = (0.01, 0.02, 0.05)[i % 3]
        if i == 0:  # dense: ns / face voxels above 0.5
            lut = 0.05
            tgt, src, _, _ = fg.synth.make_pair(8000, 6000, (1.0, 0.8, 0.6), seed=999, angle_deg=30.0)
        mse = (1e-3, 2e-3)[i % 2]
        out.append((tgt, src, lut, mse))
    return out


def _solo(fg, pairs, schedule, round_width):
    res = []
    layouts = set()
    for tgt, src, lut, mse in pairs:
        s = fg.FastGoICP(tgt, src, lut, mse, schedule=schedule, round_width=round_width)
        layouts.add(s.registration.info()["lut_layout"])
        R, t = s.run()
        res.append((R, t, s.get_best_error(), s.stats()))
        s.close()
    return res, layouts


def _check(batch, out, solo, idx):
    """batch pair k (out[k]) against solo result idx[k] (None: not compared)"""
    for k, i in enumerate(idx):
        if i is None:
            continue
        R, t, e, st = solo[i]
        assert out[k] is not None, (k, batch.status(k))
        Rb, tb = out[k]
        assert np.array_equal(Rb.view(np.uint32), R.view(np.uint32)), k
        assert np.array_equal(tb.view(np.uint32), t.view(np.uint32)), k
        assert np.float32(batch.get_best_error(k)).view(np.uint32) == np.float32(e).view(np.uint32), k
        sb = batch.stats(k)
        for key in CONTRACT:
            assert sb[key] == st[key], (k, key, sb[key], st[key])


@pytest.mark.parametrize("schedule,round_width", [(0, 1), (1, 0)], ids=["serial", "round-adaptive"])
def test_batch_matches_solo_runs_bit_for_bit(fg, schedule, round_width):
    pairs = _pairs(fg)
    solo, layouts = _solo(fg, pairs, schedule, round_width)
    assert {1, 4} <= layouts, layouts  # both packed LUT layouts in one tick
    b = fg.FastGoICPBatch(pairs, schedule=schedule, round_width=round_width)
    out = b.run()
    _check(b, out, solo, range(len(pairs)))
    bl, il = b.launches()
    assert bl > 0 and il > 0


def test_window_and_order_do_not_matter(fg):
    pairs = _pairs(fg, n=8, seed=1)
    solo, _ = _solo(fg, pairs, 1, 0)
    for max_live in (1, 3, 0):
        b = fg.FastGoICPBatch(pairs, schedule=1, round_width=0, max_live=max_live)
        _check(b, b.run(), solo, range(len(pairs)))
        b.close()
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    b = fg.FastGoICPBatch([pairs[i] for i in perm], schedule=1, round_width=0, max_live=3)
    _check(b, b.run(), solo, perm)


def test_a_pair_that_cannot_be_served_leaves_the_others_untouched(fg):
    pairs = _pairs(fg, n=5, seed=2)
    solo, _ = _solo(fg, pairs, 0, 1)
    tgt, src, _, _ = pairs[1]
    bad = (tgt, src, 1e-4, 1e-3)  # LUT dims above 4094 per axis
    b = fg.FastGoICPBatch(pairs[:2] + [bad] + pairs[2:], schedule=0, max_live=2)
    out = b.run()
    assert out[2] is None and b.status(2) == ERR_INVALID_ARG
    _check(b, out, solo, [0, 1, None, 2, 3, 4])
    with pytest.raises(fg.FgoicpError):
        b.get_best_error(2)


def test_bounds_launches_are_fused(fg):
    rng = np.random.default_rng(3)
    pairs = []
    for i in range(16):
        tgt, src, _, _ = fg.synth.make_pair(2000, 1000, (1.0, 0.8, 0.6), seed=300 + i, angle_deg=float(rng.uniform(10, 60)))
        pairs.append((tgt, src, 0.02, 1e-3))
    most = 0
    for tgt, src, lut, mse in pairs:
        s = fg.FastGoICP(tgt, src, lut, mse, schedule=1, round_width=0, flags=fg.FLAG_PROFILE)
        s.run()
        most = max(most, s.registration.profile()["launches"])
        s.close()
    b = fg.FastGoICPBatch(pairs, schedule=1, round_width=0)
    assert all(o is not None for o in b.run())
    bl, _ = b.launches()
    assert 0 < bl <= 2 * most, (bl, most)


def _write_txt(path, pts):
    with open(path, "w") as f:
        f.write(f"{len(pts)}\n")
        for x, y, z in pts:
            f.write(f"{x:.9g} {y:.9g} {z:.9g}\n")


def test_cli_batch_writes_what_lone_runs_write(fg, tmp_path):
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fast-go-icp_amd", "lib", "fast-go-icp")
    (tmp_path / "cfgs").mkdir()
    names = []
    for i, (tgt, src, lut, mse) in enumerate(_pairs(fg, n=2, seed=4)):
        _write_txt(tmp_path / f"tgt{i}.txt", tgt)
        _write_txt(tmp_path / f"src{i}.txt", src)
        for tag in ("lone", "batch"):
            (tmp_path / "cfgs" / f"{tag}{i}.toml").write_text(
                f'[io]\ntarget = "{tmp_path}/tgt{i}.txt"\nsource = "{tmp_path}/src{i}.txt"\noutput = "{tmp_path}/{tag}{i}.toml"\n'
                f'visualization = "{tmp_path}/{tag}{i}.ply"\n[params]\nlut_resolution = {lut}\nmse_threshold = {mse}\nseed = 3\n')
        names.append(f"cfgs/batch{i}.toml")
        p = subprocess.run([exe, "-c", str(tmp_path / "cfgs" / f"lone{i}.toml")], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    p = subprocess.run([exe, "--batch", str(tmp_path / "list.txt")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    for i in range(2):
        lone = [ln for ln in (tmp_path / f"lone{i}.toml").read_text().splitlines() if not ln.startswith("seconds")]
        bat = [ln for ln in (tmp_path / f"batch{i}.toml").read_text().splitlines() if not ln.startswith("seconds")]
        assert lone == bat, (lone, bat)
        assert (tmp_path / f"lone{i}.ply").read_bytes() == (tmp_path / f"batch{i}.ply").read_bytes()
    for bad in (["--batch", str(tmp_path / "list.txt"), "-c", str(tmp_path / "cfgs" / "lone0.toml")], ["--batch", str(tmp_path / "list.txt"), "--gpus", "2"]):
        assert subprocess.run([exe, *bad], capture_output=True, text=True, timeout=60).returncode != 0
