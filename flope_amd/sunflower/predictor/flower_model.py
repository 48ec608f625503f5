"""Drop-in for the reference's ``sunflower/predictor/flower_model.py`` (``FlowerModel``, :29-255;
``get_kalman_filter``, :18-26): the multi-frame step right after the pose hot path.

    add_data(rgb, depth, cam_pose[7]) -> per-frame flower poses in the camera frame (the hot path),
    moved to the world frame (cam_pose @ pose), turned into 7-vectors [x y z | qx qy qz qw] and
    associated to tracks by nearest translation (50 mm gate); every track is a 7-state
    identity-model Kalman filter whose quaternion part is re-normalised after each update.

Host-side control logic (tens of 7x7 operations per frame) and therefore plain numpy, as in the
reference.  What is deliberately kept from the reference, quirks included:
  * distances are measured to ``self.state`` -- the FIRST measurement of each track, which is never
    overwritten by the filter (flower_model.py:180-185, :211); the filtered values live in ``self.kfs``;
  * ``add_data(..., ignore=True)`` is what feeds the tracker; the default ``ignore=False`` only returns the
    per-frame poses (:244-245);
  * every measurement of a frame is matched against the tracks independently (two detections may update
    the same track in one frame), and an unmatched one opens a new track that later detections of the same
    frame cannot match (the distance matrix is computed once per frame, :181).
What is not reproduced: the matplotlib live plots (``get_plots``; display code) and the hard-coded
checkpoint / intrinsics paths -- the pose predictor is passed in.

The reference takes its filter from ``filterpy==1.4.5`` (not vendored).  ``KalmanFilter7`` restates
that class's published predict / update for the only configuration the reference uses
(F = H = I, Q = 1e-3 I, R = 0.1 I, P0 = I): predict  x <- F x, P <- F P F^T + Q;
update  y = z - H x, S = H P H^T + R, K = P H^T S^-1, x <- x + K y, P <- (I-KH) P (I-KH)^T + K R K^T.
"""
import numpy as np

from sunflower.utils.conversion import qvec2rotmat, rotmat2qvec
from sunflower.utils.mvg import pose_cam_to_world


class KalmanFilter7:
    """The subset of filterpy.kalman.KalmanFilter the reference touches: x, F, H, P, Q, R, predict(), update(z)."""

    def __init__(self, dim_x=7, dim_z=7):
        self.x = np.zeros(dim_x)
        self.F = np.eye(dim_x)
        self.H = np.eye(dim_z, dim_x)
        self.P = np.eye(dim_x)
        self.Q = np.eye(dim_x)
        self.R = np.eye(dim_z)

    def predict(self):
        self.x = self.F @ self.x
        self.P = self.F @ self.P @ self.F.T + self.Q

    def update(self, z):
        z = np.asarray(z, dtype=np.float64)
        y = z - self.H @ self.x
        PHT = self.P @ self.H.T
        S = self.H @ PHT + self.R
        K = PHT @ np.linalg.inv(S)
        self.x = self.x + K @ y
        I_KH = np.eye(self.P.shape[0]) - K @ self.H
        self.P = I_KH @ self.P @ I_KH.T + K @ self.R @ K.T


def get_kalman_filter(initial_value):
    kf = KalmanFilter7(dim_x=7, dim_z=7)
    kf.x = np.array(initial_value, dtype=np.float64)
    kf.F = np.eye(7)
    kf.H = np.eye(7)
    kf.P = np.eye(7)
    kf.Q = np.eye(7) * 0.001
    kf.R = np.eye(7) * 0.1
    return kf


def cam_pose_to_matrix(cam_pose):
    """[tx ty tz qx qy qz qw] -> 4x4 camera pose (flower_model.py:224-227)"""
    cam_pose = np.asarray(cam_pose, dtype=np.float64)
    m = np.eye(4)
    m[:3, :3] = qvec2rotmat(cam_pose[3:])
    m[:3, 3] = cam_pose[:3]
    return m


def poses_to_measurements(flower_pose_world):
    """(N,4,4) world poses -> (N,7) rows [translation, scalar-last quaternion] (flower_model.py:238-242)"""
    p = np.asarray(flower_pose_world)
    return np.hstack((p[:, :3, 3], rotmat2qvec(p[:, :3, :3])))


class FlowerModel:
    def __init__(self, dist_th=50, intrin_path=None, get_plots=False, pose_predictor=None, tracker="host", track_stream=None, track_source="measurement"):
        """tracker: "host" (default) = the reference's numpy tracker below; "device" = the same association and filters with the
        state in GPU memory (flope_amd.track.DeviceTracker): `state`, `scores`, `get_state()` and `filtered_state()`
        read from it, `add_stream` feeds it behind the frame's pose kernels without the host touching a pose, and `kfs` (the 7 x 7
        filter objects) is not offered.
        track_stream (tracker="device" only): a device-positioned encoder stream
        (`enc.open_stream(..., window=W, positions="device")`).  `add_poses(..., ignore=True)` then steps it right behind the tracker's
        update, on the device and without a host wait -- one token per track the frame touched, its `track_source` ("measurement" or
        "mean") -- and keeps the encoder's rows as `track_rows` (a device tensor [n, out_dim], row m for measurement m) and which row
        fed which track as `track_feed` ((tracks_or_codes, positions), read back only when asked for)."""
        if get_plots:
            raise NotImplementedError("the live matplotlib plots of the reference are display code and are not reproduced")
        if tracker not in ("host", "device"):
            raise ValueError(f"FlowerModel: tracker must be 'host' or 'device', got {tracker!r}")
        self.get_plots = False
        self.tracker = tracker
        self._device_tracker = None
        if track_stream is not None and tracker != "device":
            raise ValueError("FlowerModel: track_stream needs tracker='device' (the host tracker keeps no association on the device)")
        if track_stream is not None and getattr(track_stream, "positions_on", None) != "device":
            raise ValueError("FlowerModel: track_stream must be a device-positioned stream (enc.open_stream(..., positions='device'))")
        self.track_stream, self.track_source = track_stream, track_source
        self.track_rows = None                        # the encoder's rows of the last frame that fed track_stream
        if tracker == "host":
            self.state = None
            self.scores = None
            self.kfs = []
        else:
            from flope_amd.track import DeviceTracker
            self._device_tracker = DeviceTracker(getattr(pose_predictor, "device", "cuda"), dist_th=dist_th)
        self.th = dist_th / 1000
        self.intrin_path = intrin_path
        self.pose_predictor = pose_predictor          # anything with get_flower_poses(rgb, depth)

    def __getattr__(self, name):
        # only reached where normal lookup fails: tracker="device" keeps no state, scores or kfs attribute of its own
        dt = self.__dict__.get("_device_tracker")
        if dt is not None and name in ("state", "scores"):
            return getattr(dt, name)
        if dt is not None and name == "kfs":
            raise AttributeError("FlowerModel(tracker='device') keeps one variance per track on the device, not 7 x 7 filter objects: "
                                 "use filtered_state() and device_tracker.p, or tracker='host'")
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    @property
    def track_feed(self):
        """(tracks_or_codes, positions) of the last frame that fed track_stream: which track row m of `track_rows` belongs to, or a
        negative code for a row that fed nothing; None before the first.  Reading it waits for that frame's kernels."""
        if self.track_stream is None or self.track_rows is None:
            return None
        return self.track_stream.last_feed()

    @property
    def device_tracker(self):
        """the DeviceTracker behind tracker="device" (None with tracker="host")"""
        return self._device_tracker

    def assign_meas_to_state(self, meas):
        if self._device_tracker is not None:
            raise RuntimeError("FlowerModel(tracker='device') takes poses, not measurements: use add_poses / add_data / add_stream")
        meas = np.asarray(meas, dtype=np.float64)
        if self.state is None:
            self.state = meas
            self.scores = np.ones(meas.shape[0])
            for each_meas in meas:
                self.kfs.append(get_kalman_filter(each_meas))
            return
        d = np.linalg.norm(meas[:, None, :3] - self.state[None, :, :3], axis=2)      # cdist(meas, state)
        min_idx = np.argmin(d, axis=1)
        good = np.min(d, axis=1) < self.th
        for i in range(meas.shape[0]):
            if good[i]:
                kf = self.kfs[min_idx[i]]
                kf.predict()
                kf.update(meas[i])
                kf.x[3:] /= np.linalg.norm(kf.x[3:])
                self.scores[min_idx[i]] += 1
            else:
                self.state = np.vstack((self.state, meas[i].reshape(1, 7)))
                self.scores = np.hstack((self.scores, np.array([1])))
                self.kfs.append(get_kalman_filter(meas[i]))

    def add_poses(self, flower_pose_cam, cam_pose, ignore=False):
        """flower_model.py:224-255 after the predictor call: camera-frame poses of one frame -> world frame -> tracker."""
        if flower_pose_cam is None:
            return None, None
        flower_pose = pose_cam_to_world(flower_pose_cam, cam_pose_to_matrix(cam_pose))
        if ignore and self._device_tracker is not None:
            self._device_tracker.update(flower_pose_cam, cam_pose)
            if self.track_stream is not None and np.asarray(flower_pose_cam).size:      # (an empty frame is no update)
                self.track_rows = self.track_stream.step_tracker(self._device_tracker, self.track_source)
        elif ignore:
            self.assign_meas_to_state(poses_to_measurements(flower_pose))
        return flower_pose_cam, flower_pose.astype(np.float32)

    def add_data(self, rgb, depth, cam_pose, ignore=False):
        if self.pose_predictor is None:
            raise RuntimeError("FlowerModel: pass pose_predictor= (PosePredictor / FastPosePredictor)")
        return self.add_poses(self.pose_predictor.get_flower_poses(rgb, depth), cam_pose, ignore)

    def add_stream(self, frames, ignore=True, detectors=2):
        """`add_data` over a stream of (rgb, depth, cam_pose) frames with the predictor's pipelined loop
        (`FastPosePredictor.iter_flower_poses`: several frames in flight on the GPU, results in frame order) instead of one
        blocking `get_flower_poses` per frame.  Same tracker updates in the same order as calling add_data frame by frame
        (build-defined convenience: the reference's loop, scripts/live_pose.py:31-41, is sequential).  Yields add_data's
        (poses in the camera frame, poses in the world frame) per frame."""
        if self.pose_predictor is None:
            raise RuntimeError("FlowerModel: pass pose_predictor= (PosePredictor / FastPosePredictor)")
        frames = list(frames)
        it = getattr(self.pose_predictor, "iter_flower_poses", None)
        if it is not None and ignore and self._device_tracker is not None:
            # the predictor's loop feeds the tracker on the device, behind each frame's pose kernels and in frame order; the host
            # only moves the poses it hands back to the world frame
            poses = it(((f[0], f[1]) for f in frames), detectors=detectors, tracker=self._device_tracker, cam_poses=[f[2] for f in frames])
            for f, pose_cam in zip(frames, poses):
                yield self.add_poses(pose_cam, f[2], False)
            return
        poses = it(((f[0], f[1]) for f in frames), detectors=detectors) if it is not None else \
            (self.pose_predictor.get_flower_poses(f[0], f[1]) for f in frames)
        for f, pose_cam in zip(frames, poses):
            yield self.add_poses(pose_cam, f[2], ignore)

    def get_state(self):
        return self.state

    def filtered_state(self):
        """(T,7) current filter means, one row per track (the reference keeps these only inside ``kfs``)."""
        if self._device_tracker is not None:
            return self._device_tracker.filtered_state()
        return np.array([kf.x for kf in self.kfs]).reshape(-1, 7)
