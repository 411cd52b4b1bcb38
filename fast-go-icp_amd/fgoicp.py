"""Python mirror of icp::FastGoICP (fgoicp/fgoicp.hpp:8-110) over the driver-level C ABI.  The
outer/inner branch-and-bound runs in host C++ inside libfgoicp_amd.so; this class only marshals."""
import ctypes as C

import numpy as np

from . import _lib
from .nodes import from_glm
from .registration import GicpRefinement, PlaneRefinement, Registration, RobustRefinement, _alignment, _cloud, _fp, _information, _loss_code


class FastGoICP:
    def __init__(self, pct, pcs, lut_resolution=0.005, mse_threshold=1e-3, schedule=_lib.SCHEDULE_SERIAL, round_width=1,
                 device=0, flags=0, trim_fraction=0.0):
        self._lib = _lib.load()
        pct, pcs = _cloud(pct), _cloud(pcs)
        self.nt, self.ns = len(pct), len(pcs)
        opts = _lib.SolverOpts(int(schedule), int(round_width), int(flags), int(device), float(trim_fraction))
        self._h = C.c_void_p()
        _lib.check(self._lib.fgoicp_solver_create(_fp(pct), self.nt, _fp(pcs), self.ns, float(lut_resolution), float(mse_threshold),
                                                  C.byref(opts), C.byref(self._h)), "fgoicp_solver_create")
        self._exchange = None  # keeps the ctypes callbacks alive

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fgoicp_solver_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_exchange(self, exchange):
        """exchange: fgoicp_amd.dist.TorchExchange (or None for single process)."""
        self._exchange = exchange
        ptr = C.byref(exchange.struct) if exchange is not None else None
        _lib.check(self._lib.fgoicp_solver_set_exchange(self._h, ptr), "fgoicp_solver_set_exchange")

    def set_early_exit(self, on=True):
        """False: every subcube is evaluated in full, as the reference does (same trajectory and result; fgoicp_solver_set_early_exit)."""
        _lib.check(self._lib.fgoicp_solver_set_early_exit(self._h, int(bool(on))), "fgoicp_solver_set_early_exit")

    def run(self):
        """-> (R (3,3), t (3,)) with t restored to the callers' frame (fgoicp.cpp:29)."""
        R = np.empty(9, np.float32); t = np.empty(3, np.float32)
        _lib.check(self._lib.fgoicp_solver_run(self._h, _fp(R), _fp(t)), "fgoicp_solver_run")
        return from_glm(R), t

    def get_best_error(self):
        v = C.c_float()
        _lib.check(self._lib.fgoicp_solver_best_error(self._h, C.byref(v)), "fgoicp_solver_best_error")
        return np.float32(v.value)

    def alignment(self):
        """EXTENSION (fgoicp_solver_alignment): the Alignment at the best transform, after run().  Indices and masks refer to the clouds as
        passed in; dist2 is in the solver's centred and scaled frame, .distances and .inlier_rmse are in the callers' units."""
        return _alignment(lambda *a: self._lib.fgoicp_solver_alignment(self._h, *a), "fgoicp_solver_alignment", self.ns, self.nt)

    def information(self, max_distance=None):
        """EXTENSION (fgoicp_solver_information): the Information at the best transform, after run(), in the callers' frame — the target
        points as passed in.  max_distance: callers' units (None: no threshold); counted are the Alignment's inliers with
        dist2 <= (float32(max_distance) * scale)^2, evaluated in float32."""
        d = float("inf") if max_distance is None else float(max_distance)
        return _information(lambda out: self._lib.fgoicp_solver_information(self._h, d, out), "fgoicp_solver_information")

    def _set_normals(self, normals, n, call, name):
        a = _cloud(normals)
        if len(a) != n:
            raise ValueError(f"normals must be ({n}, 3): one per point of the cloud as passed in")
        _lib.check(call(self._h, _fp(a)), name)

    def set_target_normals(self, normals):
        """EXTENSION (fgoicp_solver_set_target_normals): the target's normals (nt, 3), given — those of a mesh's faces (sample_mesh), for
        instance — in the order of the target as passed in; normalised on upload.  refine_plane / refine_gicp then use them and estimate
        only what is not set (k is ignored for a set that is given)."""
        self._set_normals(normals, self.nt, self._lib.fgoicp_solver_set_target_normals, "fgoicp_solver_set_target_normals")

    def set_source_normals(self, normals):
        """EXTENSION (fgoicp_solver_set_source_normals): the source's normals (ns, 3), as set_target_normals; used by refine_gicp."""
        self._set_normals(normals, self.ns, self._lib.fgoicp_solver_set_source_normals, "fgoicp_solver_set_source_normals")

    def _refine_robust(self, model, k, max_iter, conv_thr, max_distance, epsilon, loss, loss_scale):
        d = float("inf") if max_distance is None else float(max_distance)
        raw = _lib.RobustResult()
        _lib.check(self._lib.fgoicp_solver_refine_robust(self._h, model, int(k), int(max_iter), float(conv_thr), d, float(epsilon), _loss_code(loss),
                                                         0.0 if loss_scale is None else float(loss_scale), C.byref(raw)), "fgoicp_solver_refine_robust")
        return RobustRefinement(raw, model)

    def refine_plane(self, k=16, max_iter=30, conv_thr=1e-6, max_distance=None, loss=None, loss_scale=None):
        """EXTENSION (fgoicp_solver_refine_plane): point-to-plane ICP from the best transform, after run() -> PlaneRefinement with R and t
        in the callers' frame.  The target's normals are estimated from k neighbours unless the registration already has some;
        max_distance: callers' units (None: no threshold), as information() takes it.  run() and the best transform are untouched.
        loss "huber" / "cauchy" / "geman_mcclure" / "tukey" (fgoicp_solver_refine_robust): the robustly weighted loop -> RobustRefinement;
        loss_scale in the callers' units, None: estimated at the best transform."""
        if loss is not None:
            return self._refine_robust(_lib.MODEL_PLANE, k, max_iter, conv_thr, max_distance, 1e-3, loss, loss_scale)
        d = float("inf") if max_distance is None else float(max_distance)
        raw = _lib.PlaneResult()
        _lib.check(self._lib.fgoicp_solver_refine_plane(self._h, int(k), int(max_iter), float(conv_thr), d, C.byref(raw)), "fgoicp_solver_refine_plane")
        return PlaneRefinement(raw)

    def refine_gicp(self, k=16, max_iter=30, conv_thr=1e-6, max_distance=None, epsilon=1e-3, loss=None, loss_scale=None):
        """EXTENSION (fgoicp_solver_refine_gicp): Generalized ICP from the best transform, after run() -> GicpRefinement (a
        PlaneRefinement) with R and t in the callers' frame.  Whichever normal set the registration lacks is estimated from k neighbours;
        max_distance as refine_plane takes it.  run() and the best transform are untouched.  loss and loss_scale as refine_plane's."""
        if loss is not None:
            return self._refine_robust(_lib.MODEL_GICP, k, max_iter, conv_thr, max_distance, epsilon, loss, loss_scale)
        d = float("inf") if max_distance is None else float(max_distance)
        raw = _lib.PlaneResult()
        _lib.check(self._lib.fgoicp_solver_refine_gicp(self._h, int(k), int(max_iter), float(conv_thr), d, float(epsilon), C.byref(raw)), "fgoicp_solver_refine_gicp")
        return GicpRefinement(raw)

    def _transform(self, fn, name):
        R = np.empty(9, np.float32); t = np.empty(3, np.float32)
        _lib.check(fn(self._h, _fp(R), _fp(t)), name)
        return from_glm(R), t

    def get_best_transform(self):
        return self._transform(self._lib.fgoicp_solver_best_transform, "fgoicp_solver_best_transform")

    def get_last_transform(self):
        return self._transform(self._lib.fgoicp_solver_last_transform, "fgoicp_solver_last_transform")

    def stats(self):
        st = _lib.RunStats()
        _lib.check(self._lib.fgoicp_solver_stats(self._h, C.byref(st)), "fgoicp_solver_stats")
        return st.as_dict()

    def preproc(self):
        offs = np.empty(6, np.float32); scale = C.c_float(); b = np.empty(6, np.float32)
        _lib.check(self._lib.fgoicp_solver_preproc(self._h, _fp(offs), C.byref(scale), _fp(b)), "fgoicp_solver_preproc")
        return dict(offset_pcs=offs[:3].copy(), offset_pct=offs[3:].copy(), scale=np.float32(scale.value), bounds=b.reshape(3, 2))

    @property
    def registration(self):
        """The operator context the solver drives (borrowed)."""
        return Registration._borrow(self._lib.fgoicp_solver_ctx(self._h), self)
