"""DeviceTracker: Python owner of one ``flope_track_handle`` (include/flope_amd.h, csrc/track.hip) -- the multi-frame step of
``FlowerModel`` (sunflower/predictor/flower_model.py: camera -> world, quaternion, nearest-anchor association under a gate, one
7-state Kalman filter per track) with its state in device memory.  ``update`` enqueues two launches on the current
stream and returns; only the readers wait.  PyTorch lends device pointers and the current stream."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .engine import _stream_ptr

ASSOC_SKIPPED = -2 ** 31          # an entry of last_association(): the row was unreliable and took no part


def cam_matrix16(cam_pose) -> np.ndarray:
    """the reference's camera 7-vector [tx ty tz qx qy qz qw] (or a 4x4 matrix) -> contiguous float64 [16], row-major"""
    cam = np.asarray(cam_pose, dtype=np.float64)
    if cam.shape != (4, 4):
        from sunflower.predictor.flower_model import cam_pose_to_matrix
        cam = cam_pose_to_matrix(cam.reshape(7))
    return np.ascontiguousarray(cam, dtype=np.float64).reshape(16)


class DeviceTracker:
    def __init__(self, device="cuda", max_tracks: int = 4096, max_meas: int = 300, dist_th: float = 50, q: float = 1e-3, r: float = 0.1,
                 p0: float = 1.0):
        """dist_th in millimetres, as FlowerModel's; q, r, p0: the filter's Q = q I, R = r I, P0 = p0 I"""
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("flope_amd: DeviceTracker runs on HIP devices only (there is no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)   # (without a device the create below says so)
        self.max_tracks, self.max_meas = int(max_tracks), int(max_meas)
        h = C.c_void_p()
        rc = self.lib.flope_track_create(self.device.index, self.max_tracks, self.max_meas, float(dist_th) / 1000, float(q), float(r), float(p0), C.byref(h))
        if rc != 0:
            raise RuntimeError(f"flope_track_create: {(self.lib.flope_track_last_error(None) or b'').decode()}")
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self.lib.flope_track_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> int:
        if rc < 0:
            raise RuntimeError((self.lib.flope_track_last_error(self.handle) or b"").decode() or f"flope_track error {rc}")
        return rc

    def update(self, poses, cam_pose, reliable=None) -> None:
        """poses: [n,4,4] in the camera frame, a float32 / float64 tensor on the tracker's device or a numpy array (uploaded as it
        is when float32, as float64 otherwise); cam_pose: the reference's 7-vector (or a 4x4 matrix); reliable: int32 [n] on the device
        or a numpy array, rows with 0 are skipped.  Asynchronous on the current stream; None or an empty batch is a no-op."""
        if poses is None:
            return
        if not isinstance(poses, torch.Tensor):
            poses = np.asarray(poses)
            # (a copy of its own: the caller's array may be read-only, which torch.from_numpy does not take silently)
            poses = torch.from_numpy(np.array(poses, dtype=np.float32 if poses.dtype == np.float32 else np.float64, order="C")).to(self.device)
        if poses.numel() == 0:
            return
        if not (poses.device == self.device and poses.dtype in (torch.float32, torch.float64) and poses.is_contiguous() and poses.numel() % 16 == 0):
            raise ValueError(f"poses must be contiguous float32 / float64 [n,4,4] on {self.device}")
        n = poses.numel() // 16
        rel_ptr = None
        if reliable is not None:
            if not isinstance(reliable, torch.Tensor):
                reliable = torch.from_numpy(np.array(reliable, dtype=np.int32, order="C")).to(self.device)
            if not (reliable.device == self.device and reliable.dtype == torch.int32 and reliable.is_contiguous() and reliable.numel() == n):
                raise ValueError(f"reliable must be contiguous int32 [{n}] on {self.device}")
            rel_ptr = reliable.data_ptr()
        cam = cam_matrix16(cam_pose)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            self._check(self.lib.flope_track_update(self.handle, poses.data_ptr(), int(poses.dtype == torch.float64), rel_ptr, n, cam.ctypes.data,
                                                    _stream_ptr(self.device)))
            poses.record_stream(stream)             # (an uploaded batch is freed by the caching allocator only behind the kernels)
            if reliable is not None:
                reliable.record_stream(stream)

    def reset(self) -> None:
        self._check(self.lib.flope_track_reset(self.handle))

    @property
    def last_n(self) -> int:
        """measurements of the last update that enqueued anything, -1 when there was none since the tracker was made or reset: the
        rows TransformerEncoderStream.step_tracker returns.  Kept on the host; waits for nothing."""
        v = _lib.TrackView()
        self._check(self.lib.flope_track_device_view(self.handle, C.byref(v)))
        return int(v.n)

    @property
    def count(self) -> int:
        return self._check(self.lib.flope_track_count(self.handle))

    def read(self):
        """-> (anchors [T,7], means [T,7], p [T], hits int32 [T]) after the last update"""
        T = self.count
        a, m = np.empty((T, 7)), np.empty((T, 7))
        p, h = np.empty(T), np.empty(T, dtype=np.int32)
        if T:
            self._check(self.lib.flope_track_read(self.handle, a.ctypes.data, m.ctypes.data, p.ctypes.data, h.ctypes.data, T))
        return a, m, p, h

    @property
    def state(self):
        """FlowerModel.state: every track's first measurement [T,7]; None before the first track"""
        a = self.read()[0]
        return a if len(a) else None

    @property
    def scores(self):
        """FlowerModel.scores: measurements per track, float as the reference's; None before the first track"""
        h = self.read()[3]
        return h.astype(np.float64) if len(h) else None

    def filtered_state(self) -> np.ndarray:
        return self.read()[1]

    @property
    def p(self) -> np.ndarray:
        """the filter variance of every track (its P is p I)"""
        return self.read()[2]

    def last_association(self) -> np.ndarray:
        """test hook: int32 [n] of the last update: >= 0 matched track, -1 - t opened track t, ASSOC_SKIPPED unreliable row"""
        out = np.empty(self.max_meas, dtype=np.int32)
        n = self._check(self.lib.flope_track_read_assoc(self.handle, out.ctypes.data, self.max_meas))
        return out[:n].copy()

    def raw_state(self, rows: int):
        """test hook: (anchors, means, p, hits, [tracks, overflow flag]) -- the first `rows` rows as they are in device memory,
        whatever the flag says"""
        a, m = np.empty((rows, 7)), np.empty((rows, 7))
        p, h, c = np.empty(rows), np.empty(rows, dtype=np.int32), np.empty(2, dtype=np.int32)
        self._check(self.lib.flope_track_debug_read(self.handle, a.ctypes.data, m.ctypes.data, p.ctypes.data, h.ctypes.data, c.ctypes.data, rows))
        return a, m, p, h, c

    def sentinels_changed(self) -> int:
        """test hook: how many sentinel words behind the device arrays have changed"""
        return self._check(self.lib.flope_track_debug_sentinels(self.handle))
