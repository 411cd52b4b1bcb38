"""Many registrations on one device in one run (fgoicp_batch, include/fgoicp_amd.h).  Each pair returns exactly what FastGoICP.run()
returns for it alone with the same options; the bounds and ICP work of all live pairs is evaluated in shared launches."""
import ctypes as C

import numpy as np

from . import _lib
from .nodes import from_glm
from .registration import GicpRefinement, PlaneRefinement, RobustRefinement, _alignment, _cloud, _fp, _information, _loss_code, _model_code

_REFINE_DEFAULTS = {"model": "plane", "k": 16, "max_iter": 30, "conv_thr": 1e-6, "max_distance": None, "epsilon": 1e-3, "loss": None, "loss_scale": None}


def _refine_entries(refine, n):
    """refine= of FastGoICPBatch -> None, or a list of n entries (None, or a dict with every key of _REFINE_DEFAULTS)."""
    if refine is None:
        return None
    specs = [refine] * n if isinstance(refine, dict) else list(refine)
    if len(specs) != n:
        raise ValueError(f"refine: {len(specs)} entries for {n} pairs (one dict for all, or a list with one dict or None per pair)")
    out = []
    for i, r in enumerate(specs):
        if r is None:
            out.append(None)
            continue
        unknown = set(r) - set(_REFINE_DEFAULTS)
        if unknown:
            raise ValueError(f"refine[{i}]: unknown keys {sorted(unknown)} (the keys are {sorted(_REFINE_DEFAULTS)})")
        out.append({**_REFINE_DEFAULTS, **r})
    return out


def _refine_array(entries):
    arr = (_lib.BatchRefine * max(1, len(entries)))()
    for i, r in enumerate(entries):
        arr[i].struct_size = C.sizeof(_lib.BatchRefine)
        if r is None:
            arr[i].model = -1
            continue
        arr[i].model = _model_code(r["model"])
        arr[i].k, arr[i].max_iter, arr[i].conv_thr = int(r["k"]), int(r["max_iter"]), float(r["conv_thr"])
        arr[i].max_distance = float("inf") if r["max_distance"] is None else float(r["max_distance"])
        arr[i].epsilon = float(r["epsilon"])
        arr[i].loss = _lib.LOSS_NONE if r["loss"] is None else _loss_code(r["loss"])
        arr[i].loss_scale = 0.0 if r["loss_scale"] is None else float(r["loss_scale"])
    return arr


class FastGoICPBatch:
    """pairs: iterable of (pct, pcs), (pct, pcs, lut_resolution, mse_threshold) or (pct, pcs, lut_resolution, mse_threshold, trim_fraction);
    the defaults below apply to what a pair leaves out.  trim_fraction: as FastGoICP's, per pair (0 = untrimmed).  information: False, True
    (every pair's Information without a distance threshold) or a distance in the callers' units.  refine: None, one dict for every pair, or
    a list with one dict or None per pair; the keys are model ("plane" / "gicp") and the arguments of FastGoICP.refine_plane / refine_gicp
    with their defaults: k, max_iter, conv_thr, max_distance, epsilon, loss, loss_scale (loss None or "none": the plain refinement)."""

    def __init__(self, pairs, lut_resolution=0.005, mse_threshold=1e-3, schedule=_lib.SCHEDULE_SERIAL, round_width=1, device=0, flags=0,
                 max_live=0, trim_fraction=0.0, alignment=False, information=False, refine=None):
        self._lib = _lib.load()
        self._clouds = []
        self._sizes = []
        arr = (_lib.BatchPair * max(1, len(pairs)))()
        trim = np.zeros(max(1, len(pairs)), np.float32)
        for i, p in enumerate(pairs):
            pct, pcs = _cloud(p[0]), _cloud(p[1])
            lr, mt = (p[2], p[3]) if len(p) > 2 else (lut_resolution, mse_threshold)
            trim[i] = p[4] if len(p) > 4 else trim_fraction
            self._clouds.append((pct, pcs))  # the library copies them at create; kept until then
            self._sizes.append((len(pcs), len(pct)))
            arr[i] = _lib.BatchPair(_fp(pct), len(pct), _fp(pcs), len(pcs), float(lr), float(mt))
        self.n = len(pairs)
        self._refine = _refine_entries(refine, self.n)
        rarr = None if self._refine is None else _refine_array(self._refine)
        opts = _lib.BatchOptsRefine(C.sizeof(_lib.BatchOptsRefine), _lib.SolverOpts(int(schedule), int(round_width), int(flags), int(device), 0.0), int(max_live),
                              _fp(trim), int(bool(alignment)), int(information is not False and information is not None),
                              0.0 if isinstance(information, bool) or information is None else float(information))
        if rarr is not None:
            opts.refine = rarr
        self._h = C.c_void_p()
        _lib.check(self._lib.fgoicp_batch_create(arr, self.n, C.byref(opts), C.byref(self._h)), "fgoicp_batch_create")
        self._clouds = None
        self._status = [None] * self.n

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fgoicp_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self):
        """-> list of (R (3,3), t (3,)) per pair, t restored to the callers' frame; None for a pair that could not be served (see status(i))."""
        R = np.zeros(9 * self.n, np.float32); t = np.zeros(3 * self.n, np.float32); st = np.zeros(self.n, np.int32)
        _lib.check(self._lib.fgoicp_batch_run(self._h, _fp(R), _fp(t), st.ctypes.data_as(_lib.c_int_p)), "fgoicp_batch_run")
        self._status = [int(s) for s in st]
        return [None if st[i] else (from_glm(R[9 * i:9 * i + 9]), t[3 * i:3 * i + 3].copy()) for i in range(self.n)]

    def status(self, i):
        """fgoicp_status of pair i in the last run (0 = OK)."""
        return self._status[i]

    def get_best_error(self, i):
        v = C.c_float()
        _lib.check(self._lib.fgoicp_batch_best_error(self._h, int(i), C.byref(v)), "fgoicp_batch_best_error")
        return np.float32(v.value)

    def stats(self, i):
        st = _lib.RunStats()
        _lib.check(self._lib.fgoicp_batch_stats(self._h, int(i), C.byref(st)), "fgoicp_batch_stats")
        return st.as_dict()

    def alignment(self, i):
        """EXTENSION (fgoicp_batch_alignment; needs alignment=True): pair i's Alignment at its best transform, what FastGoICP.alignment()
        returns for that pair alone."""
        ns, nt = self._sizes[i]
        return _alignment(lambda *a: self._lib.fgoicp_batch_alignment(self._h, int(i), *a), "fgoicp_batch_alignment", ns, nt)

    def information(self, i):
        """EXTENSION (fgoicp_batch_information; needs information=True or a distance): pair i's Information at its best transform, what
        FastGoICP.information(distance) returns for that pair alone."""
        return _information(lambda out: self._lib.fgoicp_batch_information(self._h, int(i), out), "fgoicp_batch_information")

    def refined(self, i):
        """EXTENSION (fgoicp_batch_refined_plane / _robust; needs refine=): pair i's refinement from its best transform, the object
        FastGoICP.refine_plane / refine_gicp returns for that pair alone with the same arguments."""
        r = self._refine[i] if self._refine is not None else None
        model = _lib.MODEL_PLANE if r is None else _model_code(r["model"])
        if r is not None and r["loss"] is not None and _loss_code(r["loss"]) != _lib.LOSS_NONE:
            raw = _lib.RobustResult()
            _lib.check(self._lib.fgoicp_batch_refined_robust(self._h, int(i), C.byref(raw)), "fgoicp_batch_refined_robust")
            return RobustRefinement(raw, model)
        raw = _lib.PlaneResult()
        _lib.check(self._lib.fgoicp_batch_refined_plane(self._h, int(i), C.byref(raw)), "fgoicp_batch_refined_plane")
        return GicpRefinement(raw) if model == _lib.MODEL_GICP else PlaneRefinement(raw)

    def refined_information(self, i):
        """EXTENSION (fgoicp_batch_refined_information; needs information= and refine=): pair i's Information at its REFINED pose;
        information(i) stays the search's."""
        return _information(lambda out: self._lib.fgoicp_batch_refined_information(self._h, int(i), out), "fgoicp_batch_refined_information")

    def refine_launches(self):
        """-> (fused refinement moment launches, refinement evaluations) of the last run."""
        b = C.c_uint64(); c = C.c_uint64()
        _lib.check(self._lib.fgoicp_batch_refine_launches(self._h, C.byref(b), C.byref(c)), "fgoicp_batch_refine_launches")
        return int(b.value), int(c.value)

    def launches(self):
        """-> (fused bounds launches, lock-step ICP iterations) of the last run."""
        b = C.c_uint64(); c = C.c_uint64()
        _lib.check(self._lib.fgoicp_batch_launches(self._h, C.byref(b), C.byref(c)), "fgoicp_batch_launches")
        return int(b.value), int(c.value)
