"""Host-side mirror of Estimator::EstimateLidarPose (Estimator.cpp:967-1140) for the live 1-frame mode: down-sample,
Estimate against the local map, hand the pose back, apply the key-scan rule and grow the local map.  Every stage
that touches points runs on the device through the C-ABI (mml_downsample, mml_estimate, mml_map_increment_local;
for n sequences in one context: the same with map banks, mml_slot_bind_bank and mml_map_bank_increment);
this file only carries the control flow and the 4x4 / quaternion bookkeeping the reference does in Eigen.

global_map=True adds the second map of an Estimator, the MAP_MANAGER cube store that Estimator::threadMapIncrement
(Estimator.cpp:92-145) feeds (mml_map_global_append / _increment, per bank mml_map_bank_global_append / _increment).  The
reference runs that thread asynchronously at 10 Hz; the schedule here is the deterministic one the thread follows when it keeps
up with the scans: every hand-off (:1070-1077) is taken before the next scan arrives.  After the pose hand-back, when the scan is
not degenerate and its down-sampled corner stack is not empty (:103): append(slot, T), map_update_ID += 1, and MapIncrement at T
when map_update_ID % map_skip_frame == 0.  Estimate then matches a feature against its cube first (the copy taken at the start of
the last MapIncrement) and falls back to the local map, and the gate in front of Estimate is the whole of :1032-1035.
"""
import numpy as np


def _quat_to_matrix(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


# ---- the per-sequence host steps of EstimateLidarPose, shared by LidarOdometry and BatchLidarOdometry.  `st` is whatever carries
# one Estimator's bookkeeping as attributes (_sequence_init): the LidarOdometry itself, or one sequence of the batch class.
def _sequence_init(st):
    st.last_velo_update_pose = np.array([-1.0, -1.0, -1.0])       # Estimator.h:339-340
    st.last_hori_update_pose = np.array([-1.0, -1.0, -1.0])
    st.n_corner_local = 0
    st.n_surf_local = 0
    st.fail_detected = False
    st.key_scans = 0
    st.n_corner_global = 0                                        # laserCloud{Corner,Surf}FromMapNum: the last MapIncrement's sizes
    st.n_surf_global = 0
    st.map_update_id = 0                                          # map_update_ID, Estimator.h:332
    st.last_T = None                                              # transformTobeMapped the last estimate_lidar_pose ended with


def _transform_to_be_mapped(exRbl, exPbl, P, Q):
    T = np.eye(4)
    R = _quat_to_matrix(Q)
    T[:3, :3] = R @ exRbl
    T[:3, 3] = R @ exPbl + P
    return T


def _local_map_gate(st):
    """:1032-1035 (local-map half of the gate): Estimate runs only against a local map that holds something."""
    return st.n_corner_local > 0 and st.n_surf_local > 100


def _map_gate(st):
    """:1032-1035, the whole gate: the cube store's sizes as the last MapIncrement returned them (0 without global_map), or the
    local map's."""
    return (st.n_corner_global > 0 and st.n_surf_global > 100) or _local_map_gate(st)


def _map_thread_takes(is_degenerate, n_corner_stack):
    """Whether threadMapIncrement gets this scan: handed off at all (:1070) and a corner stack that is not empty (:103)."""
    return (not is_degenerate) and n_corner_stack > 0


def _map_thread_appended(st, map_skip_frame):
    """After featureAssociateToMap of a scan (:105-122): counts it; True when MapIncrement is due (:129)."""
    st.map_update_id += 1
    return st.map_update_id % map_skip_frame == 0


def _map_thread_incremented(st, sizes):
    st.n_corner_global, st.n_surf_global = int(sizes[0]), int(sizes[1])


def _hand_back(st, lidar_mode, exRbl, exPbl, T, P, Q, is_degenerate, corner_cnt):
    """The pose hand-back (:1041-1066) and the key-scan rule (:1070-1136) up to the map increment.  T: transformTobeMapped of
    the prediction; P, Q: what Estimate returned (the prediction when it did not run).  Returns (T, grow)."""
    if (lidar_mode == 1 and not is_degenerate and corner_cnt > 100) or (lidar_mode == 2 and corner_cnt > 50):
        T = _transform_to_be_mapped(exRbl, exPbl, P, Q)           # :1041-1049
    else:                                                         # :1050-1066: keep the predicted x / y, old z
        T[:3, 3] = [P[0], P[1], T[2, 3]]
    grow = False
    if not is_degenerate:                                         # :1070-1136
        # both modes compare with last_velo_update_pose (:1082, :1119); mode 1 writes last_hori_update_pose (:1115), which
        # nothing reads -- the reference's bookkeeping as it is
        d = st.last_velo_update_pose - T[:3, 3]
        dis = float(np.float32(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])) if lidar_mode == 2 else float(d @ d)
        grow = dis >= 0.5 and lidar_mode in (1, 2)
    return T, grow


def _grown(st, lidar_mode, T, sizes):
    """After MapIncrementLocal at T (:1112, :1125-1130): the new map sizes and the key-scan pose."""
    st.n_corner_local, st.n_surf_local = int(sizes[0]), int(sizes[1])
    if lidar_mode == 2:
        st.last_velo_update_pose = T[:3, 3].copy()
    else:
        st.last_hori_update_pose = T[:3, 3].copy()
    st.key_scans += 1


def _finish(st, T, is_degenerate):
    st.fail_detected = is_degenerate                              # :1139
    st.last_T = T


def _published(st, fast_rotation):
    """Whether the pose node publishes the scan's registered cloud (unionPoseEstimation.cpp:906): no failure detected by the
    estimate that just ended, and no fast rotation seen by the caller."""
    return not st.fail_detected and not fast_rotation


def _world_map_create(ctx, n, world_map):
    """world_map: None, or (leaf, capacity_voxels) -- n device-resident voxel maps of the registered clouds, one per sequence --,
    or (leaf, capacity_voxels, "surfels"): the same maps with per-voxel moments, normals and planarity (a surfel map)."""
    if world_map is None:
        return None
    if len(world_map) == 3:
        if world_map[2] != "surfels":
            raise ValueError('world_map: the third element, if given, is "surfels"')
        leaf, capacity = world_map[:2]
        ctx.world_map_create(n, leaf, capacity, surfels=True)
        return float(leaf), int(capacity), "surfels"
    leaf, capacity = world_map
    ctx.world_map_create(n, leaf, capacity)
    return float(leaf), int(capacity)


def _world_map_download(od, n, seq, surfels=False):
    if not od._world_map:
        raise ValueError("no world map: pass world_map=(leaf, capacity_voxels)")
    if surfels and len(od._world_map) != 3:
        raise ValueError('no surfel map: pass world_map=(leaf, capacity_voxels, "surfels")')
    if not 0 <= seq < n:
        raise ValueError("sequence %d outside [0, %d)" % (seq, n))
    return od.ctx.world_map_surfels(seq) if surfels else od.ctx.world_map_download(seq)


def _world_map_roll_init(od, world_map_roll, on_evict):
    """world_map_roll: None, or (half_extent_xyz_m, every) -- after the world-map add of every `every`-th round ONE
    Context.world_map_evict for all sequences removes, from each sequence's map, the voxels outside the box of that half extent
    (one value or three, metres) around the sequence's current position; their rows go to on_evict(seq, rows) when given (rows as
    Context.world_map_import takes them) and are dropped otherwise."""
    od._roll = None
    if world_map_roll is None:
        if on_evict is not None:
            raise ValueError("on_evict needs world_map_roll=(half_extent_xyz_m, every)")
        return
    if not od._world_map:
        raise ValueError("world_map_roll needs world_map=(leaf, capacity_voxels)")
    half, every = world_map_roll
    half = np.broadcast_to(np.asarray(half, dtype=np.float64), (3,)).copy()
    if not (np.isfinite(half).all() and (half > 0).all()) or int(every) != every or every < 1:
        raise ValueError("world_map_roll: a finite positive half extent and every >= 1")
    od._roll, od._on_evict, od._roll_rounds = (half, int(every)), on_evict, 0


def _world_map_rolled(od, last_T):
    """The end of a round: last_T[w] is sequence w's lidar pose, None while it has none."""
    if od._roll is None:
        return
    od._roll_rounds += 1
    half, every = od._roll
    if od._roll_rounds % every:
        return
    from . import WM_EVICT_OUTSIDE, wm_evict_rule
    rules = []
    for w, T in enumerate(last_T):
        if T is not None:
            lo, hi = od.ctx.world_map_index_box(T[:3, 3] - half, T[:3, 3] + half)
            rules.append(wm_evict_rule(w, WM_EVICT_OUTSIDE, lo, hi))
    if not rules:
        return
    if od._on_evict is None:
        od.ctx.world_map_evict(rules, rows=False)
        return
    _, rows = od.ctx.world_map_evict(rules)
    for r in rules:
        od._on_evict(r.map, rows[r.map])


def _adjacent_runs(items, slot_of):
    """items sorted by slot and cut wherever the next slot is not the one after: one device call per run."""
    runs = []
    for it in sorted(items, key=slot_of):
        if runs and slot_of(it) == slot_of(runs[-1][-1]) + 1:
            runs[-1].append(it)
        else:
            runs.append([it])
    return runs


class LidarOdometry:
    """One Estimator instance: `ctx` owns the scan slots and the maps.  lidar_mode 1 = Horizon, 2 = Velodyne
    (the fused cloud is processed as mode 2, unionPoseEstimation.cpp:872).  global_map=True: the context's cube store follows
    the map thread's schedule (the module docstring: the one the reference's asynchronous thread follows when it keeps up) and
    Estimate matches against it first; the default drives the local map alone, call for call as before.
    world_map_roll=(half_extent_xyz_m, every), with world_map: the world map follows the sensor (_world_map_roll_init); the
    default None calls nothing."""

    def __init__(self, ctx, exTlb=None, lidar_mode=2, max_outer=5, inner_iters=10, global_map=False, map_skip_frame=2,
                 world_map=None, world_map_roll=None, on_evict=None):
        if map_skip_frame < 1:
            raise ValueError("map_skip_frame must be at least 1")
        self._world_map = _world_map_create(ctx, 1, world_map)
        self.ctx = ctx
        _world_map_roll_init(self, world_map_roll, on_evict)       # (_world_map_roll_init: a rolling world map)
        self.exTlb = np.eye(4) if exTlb is None else np.asarray(exTlb, dtype=np.float64)
        self.exRbl = self.exTlb[:3, :3].T.copy()                      # :973
        self.exPbl = -1.0 * self.exRbl @ self.exTlb[:3, 3]            # :974
        self.lidar_mode = lidar_mode
        self.max_outer, self.inner_iters = max_outer, inner_iters
        self.global_map, self.map_skip_frame = global_map, map_skip_frame
        _sequence_init(self)
        ctx.map_local_reset()
        if global_map:
            ctx.map_global_reset()

    def transform_to_be_mapped(self, P, Q):
        return _transform_to_be_mapped(self.exRbl, self.exPbl, P, Q)

    def estimate_lidar_pose(self, slot, P, Q, fast_rotation=False):
        """P (3), Q (x, y, z, w): predicted body pose of the scan in `slot` (already extracted and undistorted).
        Returns the estimated (P, Q) and whether the local map grew.  With world_map=(leaf, capacity_voxels) the scan goes into
        the world map when the pose node would publish it (_published; fast_rotation: the node's detected_fast_rotation)."""
        ctx = self.ctx
        P = np.asarray(P, dtype=np.float64).copy()
        Q = np.asarray(Q, dtype=np.float64).copy()
        T = self.transform_to_be_mapped(P, Q)                          # :975-977
        corner_cnt = ctx.scan_info(slot).fused_corner_num              # :990-996
        ctx.downsample(slot, 1)                                        # :1013-1024
        is_degenerate = False
        if _map_gate(self):
            Pn, Qn, info = ctx.estimate(slot, 1, self.exTlb, P[None], Q[None], self.max_outer, self.inner_iters)
            P, Q = Pn[0], Qn[0]
            is_degenerate = bool(info[0].is_degenerate)
        T, grew = _hand_back(self, self.lidar_mode, self.exRbl, self.exPbl, T, P, Q, is_degenerate, corner_cnt)
        if self.global_map and _map_thread_takes(is_degenerate, ctx.features_count(slot, 0)):
            ctx.map_global_append(slot, T)
            if _map_thread_appended(self, self.map_skip_frame):
                _map_thread_incremented(self, ctx.map_global_increment(T))
        if grew:
            _grown(self, self.lidar_mode, T, ctx.map_increment_local(slot, T))
        _finish(self, T, is_degenerate)
        if self._world_map and _published(self, fast_rotation):
            ctx.world_map_add(slot, [0], T)
        _world_map_rolled(self, [self.last_T])
        return P, Q, grew

    def world_map(self, seq=0):
        """The world map of the sequence: (n, 4) float32 voxel centroids x, y, z, intensity in ascending key order."""
        return _world_map_download(self, 1, seq)

    def world_map_surfels(self, seq=0):
        """The surfels of the sequence's world map (world_map=(leaf, capacity_voxels, "surfels")), row for row the voxels of
        world_map(): (n, 8) float32 nx ny nz | l0 l1 l2 | planarity linearity."""
        return _world_map_download(self, 1, seq, surfels=True)

    def registered_cloud(self, slot):
        """The scan of `slot` in the world frame at the pose the last estimate_lidar_pose ended with -- the cloud the pose node
        publishes after EstimateLidarPose (unionPoseEstimation.cpp:896-911) -- as (n, 12) float32 PointXYZINormal records,
        transformed and packed on the device."""
        if self.last_T is None:
            raise ValueError("registered_cloud needs an estimate_lidar_pose first")
        return self.ctx.cloud_download_registered(slot, 1, self.last_T)[0]


class _Sequence:
    """The bookkeeping of one sequence of a BatchLidarOdometry (the attributes _sequence_init sets)."""

    def __init__(self):
        _sequence_init(self)


class BatchLidarOdometry:
    """n LidarOdometry loops in lockstep in ONE context -- a fleet's bags, or one bag cut into segments, replayed offline.
    Sequence w owns map bank w (Context.map_banks(n), created here; the context's own map is not used), so every sequence is
    matched against and grows its own local map.  Per round of scans: one bind_banks and one downsample call per run of
    adjacent slots, one estimate call per run of adjacent slots among the sequences whose bank passes the local-map gate, the
    pose hand-back and the key-scan rule per sequence on the host (the functions LidarOdometry calls), and ONE bank_increment
    call for the sequences that grew.  Every sequence reproduces what a LidarOdometry of its own on a fresh context produces.
    The per-sequence state is in self.seq[w] (n_corner_local, n_surf_local, key_scans, fail_detected, last_T, ...).
    global_map=True: bank w also keeps sequence w's cube store and match copy, on the map thread's schedule of the module
    docstring (the one the reference's asynchronous thread follows when it keeps up): per round ONE bank_global_append call for
    the sequences whose scan the thread takes and ONE bank_global_increment call for those whose MapIncrement is due.  The
    context's OWN global cube map must stay unset either way: a bound slot and it exclude each other.
    increment: "loop" (the default) -- bank_increment works the growing banks through one after the other; "segmented" -- it
    works them in one chain of launches (Context.bank_increment(..., segmented=True)): the same maps bit for bit, 2 + R host
    synchronisations per round whatever n is.
    global_increment: the same choice for the two cube calls of a round (global_map=True): "loop" (the default) or "segmented"
    (Context.bank_global_append / bank_global_increment with segmented=True): the same stores and match copies bit for bit,
    3 + R host synchronisations per round whatever n is.
    world_map_roll=(half_extent_xyz_m, every), with world_map: after the add of every `every`-th round ONE world_map_evict for all
    sequences keeps each map to a box around its sequence's position (_world_map_roll_init); the default None calls nothing."""

    def __init__(self, ctx, n, exTlb=None, lidar_mode=2, max_outer=5, inner_iters=10, global_map=False, map_skip_frame=2,
                 increment="loop", global_increment="loop", world_map=None, world_map_roll=None, on_evict=None):
        if n < 1:
            raise ValueError("n must be at least 1")
        self._world_map = _world_map_create(ctx, n, world_map)
        self.ctx = ctx
        _world_map_roll_init(self, world_map_roll, on_evict)       # (_world_map_roll_init: rolling world maps)
        if map_skip_frame < 1:
            raise ValueError("map_skip_frame must be at least 1")
        if increment not in ("loop", "segmented"):
            raise ValueError('increment must be "loop" or "segmented"')
        if global_increment not in ("loop", "segmented"):
            raise ValueError('global_increment must be "loop" or "segmented"')
        self.increment = increment
        self.global_increment = global_increment
        self.global_map, self.map_skip_frame = global_map, map_skip_frame
        self.ctx, self.n = ctx, n
        self.exTlb = np.eye(4) if exTlb is None else np.asarray(exTlb, dtype=np.float64)
        self.exRbl = self.exTlb[:3, :3].T.copy()
        self.exPbl = -1.0 * self.exRbl @ self.exTlb[:3, 3]
        self.lidar_mode = lidar_mode
        self.max_outer, self.inner_iters = max_outer, inner_iters
        self.seq = [_Sequence() for _ in range(n)]
        self._bound = {}                                               # slot -> bank, as this object last bound it
        ctx.map_banks(n)

    @property
    def key_scans(self):
        return [st.key_scans for st in self.seq]

    def estimate_lidar_pose(self, slots, P, Q, fast_rotation=None):
        """slots[w]: the slot that holds sequence w's scan (already extracted and undistorted), or None when the sequence has
        no scan this round; P (n, 3), Q (n, 4; x, y, z, w): the predicted body poses.  No two sequences may share a slot.
        Returns (P, Q, grew): the estimated poses (a sequence without a scan keeps its row) and one bool per sequence.
        With world_map=(leaf, capacity_voxels), sequence w's scan goes into world map w at its transformTobeMapped when the pose
        node would publish it (_published; fast_rotation: one detected_fast_rotation flag per sequence, None = none)."""
        ctx, n = self.ctx, self.n
        if len(slots) != n:
            raise ValueError("one slot (or None) per sequence (%d)" % n)
        P = np.array(P, dtype=np.float64).reshape(n, 3)
        Q = np.array(Q, dtype=np.float64).reshape(n, 4)
        live = [w for w in range(n) if slots[w] is not None]
        if len(set(slots[w] for w in live)) != len(live):
            raise ValueError("two sequences share a slot")
        slot_of = lambda w: slots[w]
        runs = _adjacent_runs(live, slot_of)
        for run in runs:                                               # the slots' banks, where they are not bound already
            if any(self._bound.get(slots[w]) != w for w in run):
                ctx.bind_banks(slots[run[0]], run)
                self._bound.update((slots[w], w) for w in run)
        T = {w: _transform_to_be_mapped(self.exRbl, self.exPbl, P[w], Q[w]) for w in live}       # :975-977
        corner_cnt = {w: ctx.scan_info(slots[w]).fused_corner_num for w in live}                 # :990-996
        for run in runs:
            ctx.downsample(slots[run[0]], len(run))                                              # :1013-1024
        degenerate = {w: False for w in live}
        for run in _adjacent_runs([w for w in live if _map_gate(self.seq[w])], slot_of):
            Pn, Qn, info = ctx.estimate(slots[run[0]], len(run), self.exTlb, P[run], Q[run], self.max_outer, self.inner_iters)
            for i, w in enumerate(run):
                P[w], Q[w] = Pn[i], Qn[i]
                degenerate[w] = bool(info[i].is_degenerate)
        grew = [False] * n
        for w in live:
            T[w], grew[w] = _hand_back(self.seq[w], self.lidar_mode, self.exRbl, self.exPbl, T[w], P[w], Q[w], degenerate[w], corner_cnt[w])
        if self.global_map:
            ghow = {"segmented": True} if self.global_increment == "segmented" else {}     # ("loop": call for call as before)
            taken = [w for w in live if _map_thread_takes(degenerate[w], ctx.features_count(slots[w], 0))]
            if taken:
                ctx.bank_global_append(taken, [slots[w] for w in taken], np.stack([T[w] for w in taken]), **ghow)
            due = [w for w in taken if _map_thread_appended(self.seq[w], self.map_skip_frame)]
            if due:
                nc, ns = ctx.bank_global_increment(due, np.stack([T[w] for w in due]), **ghow)
                for i, w in enumerate(due):
                    _map_thread_incremented(self.seq[w], (nc[i], ns[i]))
        growing = [w for w in live if grew[w]]
        if growing:
            how = {"segmented": True} if self.increment == "segmented" else {}    # ("loop": call for call as before)
            nc, ns = ctx.bank_increment(growing, [slots[w] for w in growing], np.stack([T[w] for w in growing]), **how)
            for i, w in enumerate(growing):
                _grown(self.seq[w], self.lidar_mode, T[w], (nc[i], ns[i]))
        for w in live:
            _finish(self.seq[w], T[w], degenerate[w])
        if self._world_map:                                            # one add per run of adjacent slots among the published scans
            fast = [False] * n if fast_rotation is None else list(fast_rotation)
            for run in _adjacent_runs([w for w in live if _published(self.seq[w], fast[w])], slot_of):
                ctx.world_map_add(slots[run[0]], run, np.stack([T[w] for w in run]))
        _world_map_rolled(self, [st.last_T for st in self.seq])
        return P, Q, grew

    def world_map(self, seq):
        """The world map of sequence `seq`: (n, 4) float32 voxel centroids x, y, z, intensity in ascending key order."""
        return _world_map_download(self, self.n, seq)

    def world_map_surfels(self, seq):
        """The surfels of sequence `seq`'s world map (world_map=(leaf, capacity_voxels, "surfels")), row for row the voxels of
        world_map(seq): (n, 8) float32 nx ny nz | l0 l1 l2 | planarity linearity."""
        return _world_map_download(self, self.n, seq, surfels=True)


def _rotvec_from_quat(q):
    """Sophus::SO3d(Q).log() (vector2double, Estimator.cpp:942)."""
    x, y, z, w = q
    n = np.sqrt(x * x + y * y + z * z)
    if n < 1e-10:
        k = 2.0 / w - (2.0 / 3.0) * n * n / (w * w * w)
    elif abs(w) < 1e-10:
        k = (np.pi if w > 0 else -np.pi) / n
    else:
        k = 2.0 * np.arctan(n / w) / n
    return np.array([k * x, k * y, k * z])


def _quat_from_rotvec(phi):
    """Sophus::SO3d::exp(phi).unit_quaternion() (double2vector, Estimator.cpp:958)."""
    th = np.linalg.norm(phi)
    if th * th < 1e-20:
        im, re = 0.5 - th * th / 48.0, 1.0 - th * th / 8.0
    else:
        im, re = np.sin(0.5 * th) / th, np.cos(0.5 * th)
    return np.array([im * phi[0], im * phi[1], im * phi[2], re])


def _pack_state(frames):
    """vector2double: one row [P | rotation vector | V | bg | ba] per frame."""
    return np.stack([np.concatenate([fr["P"], _rotvec_from_quat(fr["Q"]), fr["V"], fr["bg"], fr["ba"]]) for fr in frames])


def _unpack_state(frames, x):
    """double2vector: the rows of x back into the frame dicts."""
    for f, fr in enumerate(frames):
        fr["P"], fr["Q"] = x[f][0:3].copy(), _quat_from_rotvec(x[f][3:6])
        fr["V"], fr["bg"], fr["ba"] = x[f][6:9].copy(), x[f][9:12].copy(), x[f][12:15].copy()


def _outer_converged(q_before, t_before, frame):
    """The outer loop's stopping test on the newest frame (Estimator.cpp:1443-1447)."""
    d = abs(float(np.dot(q_before, frame["Q"])))
    deltaR = 2.0 * np.arccos(min(1.0, d)) * 180.0 / np.pi      # angularDistance, :1443
    deltaT = float(np.linalg.norm(t_before - frame["P"]))
    return deltaR < 0.05 and deltaT < 0.05


def _consecutive(slots):
    return all(s == slots[0] + f for f, s in enumerate(slots))


def _new_solver(M, W, inner_iters, w_tan, preints, gravity, prior):
    """The problem of one outer iteration: IMU factors preints[1 .. W-1], the prior when there is one."""
    fw = M.FullWindowSolver(W, max_iters=inner_iters, fixed=False, huber=0.0, w_tan=w_tan)
    for f in range(1, W):
        fw.set_imu(f, preints[f], gravity)
    if prior is not None:
        fw.set_prior(prior)
    return fw


class MapLocalizer:
    """Scans registered against a finished surfel world map of the context (Context.world_map_create(..., surfels=True), filled
    by world_map_add or world_map_import): localize(slots, P, Q) runs ONE mml_world_map_localize for a run of consecutive slots
    whose surf stacks are down-sampled.  maps: the map of every slot of the context, or one map for all.  The maps are only
    read; a localised scan enters its map when the caller calls ctx.world_map_add."""

    def __init__(self, ctx, maps, exTlb=None, opts=None):
        self.ctx, self.maps, self.opts = ctx, maps, opts
        self.exTlb = np.eye(4) if exTlb is None else np.asarray(exTlb, np.float64).reshape(4, 4)

    def localize(self, slots, P, Q):
        """slots: consecutive slot numbers; P (n, 3), Q (n, 4): the start poses.  Returns P, Q, [EstimateInfo]."""
        slots = [int(s) for s in slots]
        if not slots or slots != list(range(slots[0], slots[0] + len(slots))):
            raise ValueError("localize takes a run of consecutive slots")
        maps = [self.maps] * len(slots) if np.isscalar(self.maps) else [self.maps[s] for s in slots]
        return self.ctx.world_map_localize(slots[0], maps, self.exTlb, P, Q, self.opts)

    def relocalize(self, slots, P, Q, opts=None):
        """The same run of slots without a good start pose: P, Q are seeds, the coarse-to-fine search of
        Context.world_map_relocalize (opts: a WmRelocOpts, None: the defaults for the map's leaf) finds the start and the loop
        above ends it.  Returns P, Q, [WmRelocInfo]."""
        slots = [int(s) for s in slots]
        if not slots or slots != list(range(slots[0], slots[0] + len(slots))):
            raise ValueError("relocalize takes a run of consecutive slots")
        maps = [self.maps] * len(slots) if np.isscalar(self.maps) else [self.maps[s] for s in slots]
        return self.ctx.world_map_relocalize(slots[0], maps, self.exTlb, P, Q, opts)


class _FullWindowBase:
    """What the two full-window estimators share: the extrinsic, the constants of Estimator::Estimate and the
    marginalization switch."""

    def __init__(self, ctx, exTlb, max_outer, inner_iters, marginalize):
        if marginalize not in ("device", "host"):
            raise ValueError("marginalize must be 'device' or 'host'")
        self.marginalize = marginalize
        import importlib
        self.M = importlib.import_module(__package__)
        self.ctx = ctx
        self.exTlb = np.eye(4) if exTlb is None else np.asarray(exTlb, dtype=np.float64)
        self.T_bl = np.linalg.inv(self.exTlb)
        self.exRbl = self.exTlb[:3, :3].T.copy()
        self.exPbl = -1.0 * self.exRbl @ self.exTlb[:3, 3]
        self.max_outer, self.inner_iters = max_outer, inner_iters
        self.plan_weight_tan = 0.0003     # :1203
        self.thres_dist = 1.0             # :1204

    def _T_wl(self, x15):
        R = _quat_to_matrix(_quat_from_rotvec(x15[3:6]))
        T = np.eye(4)
        T[:3, :3] = R @ self.exRbl
        T[:3, 3] = R @ self.exPbl + x15[:3]
        return T


class WindowEstimator(_FullWindowBase):
    """Estimator::Estimate in full-window mode (windowSize == SLIDEWINDOWSIZE, Estimator.cpp:1143-1581): lidar factors
    of every frame (associated once, thres_dist 1, plan_weight_tan 3e-4, no loss), IMU factors between consecutive
    frames, the marginalization prior of the previous call.  Association runs on the device.  solver="device" (the
    default when the window sits in consecutive slots): the 15 W trust-region iteration with its IMU factors and
    prior is one kernel launch (mml_fullwindow_solve); solver="host": the iteration is host code behind the same
    C-ABI (mml_fullwindow_step) and every evaluation fetches the per-frame lidar normal equations from the device.
    marginalize="host" (the default): frame 0's lidar record is fetched and the marginalization is host code;
    marginalize="device": one device call (mml_fullwindow_marginalize_batch, n = 1) without that round trip, the prior
    bit-identical to the host's."""

    def __init__(self, ctx, exTlb=None, gravity=(0.0, 0.0, -9.805), max_outer=5, inner_iters=10, solver="device",
                 marginalize="host"):
        if solver not in ("device", "host"):
            raise ValueError("solver must be 'device' or 'host'")
        self.solver = solver
        super().__init__(ctx, exTlb, max_outer, inner_iters, marginalize)
        self.gravity = np.asarray(gravity, dtype=np.float64)
        self.prior = None                 # last_marginalization_info

    def _records(self, slots, x):
        # one launch + one read-back per trust-region evaluation when the window sits in consecutive slots
        if _consecutive(slots):
            return self.ctx.linearize_window(slots[0], len(slots), x, self.T_bl, self.plan_weight_tan, 0.0)
        M = self.M
        return np.stack([M.pack_record(*self.ctx.linearize(s, x[f][:6], self.T_bl, self.plan_weight_tan, 0.0))
                         for f, s in enumerate(slots)])

    def estimate(self, slots, frames, preints):
        """slots: scan slot of every frame (already down-sampled); frames: list of dicts with P, Q (x,y,z,w), V, bg, ba
        (updated in place); preints[f] (f >= 1): mml_imu_preint between frames f-1 and f.  Returns the new prior."""
        M, ctx, W = self.M, self.ctx, len(slots)
        info = dict(outer=0, summaries=[])
        for it in range(self.max_outer):
            x = _pack_state(frames)
            if it == 0:                                        # vLineFeatures / vPlanFeatures are empty only here
                if _consecutive(slots):                        # one enqueue for the whole window, no read-back
                    ctx.associate(slots[0], W, np.stack([self._T_wl(x[f]) for f in range(W)]), self.thres_dist, stats=False)
                else:
                    for f, s in enumerate(slots):
                        ctx.associate(s, 1, self._T_wl(x[f])[None], self.thres_dist, stats=False)
            q_before, t_before = frames[-1]["Q"].copy(), frames[-1]["P"].copy()
            fw = _new_solver(M, W, self.inner_iters, self.plan_weight_tan, preints, self.gravity, self.prior)
            if self.solver == "device" and _consecutive(slots):
                x, _, evals = fw.solve_device(ctx, slots[0], self.T_bl, x)
                info["evaluations"] = info.get("evaluations", 0) + evals
            else:
                for _ in range(20 * self.inner_iters):
                    done, x = fw.step(self._records(slots, x), x)
                    info["evaluations"] = info.get("evaluations", 0) + 1
                    if done:
                        break
            info["summaries"].append(fw.summary())
            _unpack_state(frames, x)
            info["outer"] = it + 1
            if _outer_converged(q_before, t_before, frames[-1]) or it + 1 == self.max_outer:
                # marginalize frame 0 (:1453-1546): previous prior, IMU factor 0-1, the stored lidar factors of frame 0
                if W < 2:
                    self.prior = None
                elif self.marginalize == "device":
                    self.prior = fw.marginalize_device(ctx, slots[0], self.T_bl, x)
                else:
                    rec0 = M.pack_record(*ctx.linearize(slots[0], x[0][:6], self.T_bl, self.plan_weight_tan, 0.0))
                    self.prior = fw.marginalize(rec0, x)
                break
        return info


class BatchWindowEstimator(_FullWindowBase):
    """WindowEstimator(solver="device") for n windows at once -- a fleet's bags, or one bag cut into segments, replayed in
    full-window mode.  The outer loops of all windows run in lockstep: one association call per run of adjacent slots at
    outer iteration 0, then one mml_fullwindow_solve_batch per outer iteration over the windows that have not converged yet.
    Every window keeps its own convergence test, its own gravity and its own prior (priors[w]), so its frames, counts and
    prior equal what a WindowEstimator of its own produces on the same inputs (both classes pack, unpack, test and build
    their problems through the same module functions).  marginalize="host" (the default): the batch
    call hands back every window's frame-0 record and the windows that converge are marginalized on the host one by one;
    marginalize="device": no records come back, the windows that converge in an outer iteration are marginalized by one
    mml_fullwindow_marginalize_batch call, bit-identical priors."""

    def __init__(self, ctx, n, exTlb=None, gravity=(0.0, 0.0, -9.805), max_outer=5, inner_iters=10, marginalize="host"):
        super().__init__(ctx, exTlb, max_outer, inner_iters, marginalize)
        self.n = n
        g = np.asarray(gravity, dtype=np.float64)
        if g.shape not in ((3,), (n, 3)):
            raise ValueError("gravity must be one vector or one per window")
        self.gravity = np.broadcast_to(g, (n, 3)).copy()
        self.priors = [None] * n          # last_marginalization_info of every window

    def estimate(self, slots, frames, preints):
        """One entry per window in each list: slots[w] the (consecutive) scan slots of window w's frames, frames[w] its
        frame dicts (updated in place), preints[w][f] (f >= 1) its pre-integrations.  Windows must not share a slot (each
        is associated at its own poses).  Returns one info dict per window (outer, evaluations, summaries); the new priors
        are in self.priors."""
        M, ctx, n = self.M, self.ctx, self.n
        if not (len(slots) == len(frames) == len(preints) == n):
            raise ValueError("slots, frames and preints must have one entry per window (%d)" % n)
        for w in range(n):
            if len(slots[w]) < 1 or len(frames[w]) != len(slots[w]) or len(preints[w]) != len(slots[w]):
                raise ValueError("window %d: slots, frames and preints differ in length" % w)
            if not _consecutive(slots[w]):
                raise ValueError("window %d: its slots must be consecutive" % w)
        owner = {}
        for w in range(n):
            for f, s in enumerate(slots[w]):
                if s in owner:
                    raise ValueError("slot %d belongs to windows %d and %d" % (s, owner[s][0], w))
                owner[s] = (w, f)
        infos = [dict(outer=0, summaries=[], evaluations=0) for _ in range(n)]
        active = list(range(n))
        for it in range(self.max_outer):
            xs = [_pack_state(frames[w]) for w in active]
            if it == 0:                                        # vLineFeatures / vPlanFeatures are empty only here
                order = sorted(owner)
                run = []
                for i, s in enumerate(order):                  # one enqueue per run of adjacent slots, no read-back
                    run.append(s)
                    if i + 1 == len(order) or order[i + 1] != s + 1:
                        T = np.stack([self._T_wl(xs[owner[r][0]][owner[r][1]]) for r in run])
                        ctx.associate(run[0], len(run), T, self.thres_dist, stats=False)
                        run = []
            before = [(frames[w][-1]["Q"].copy(), frames[w][-1]["P"].copy()) for w in active]
            solvers = [_new_solver(M, len(slots[w]), self.inner_iters, self.plan_weight_tan, preints[w], self.gravity[w], self.priors[w])
                       for w in active]
            on_device = self.marginalize == "device"
            out = M.fullwindow_solve_batch(ctx, solvers, [slots[w][0] for w in active], self.T_bl, xs, records0=not on_device)
            xo, evals, rec0 = out[0], out[2], None if on_device else out[3]
            still, closing = [], []
            for i, w in enumerate(active):
                x, info = xo[i], infos[w]
                info["evaluations"] += evals[i]
                info["summaries"].append(solvers[i].summary())
                _unpack_state(frames[w], x)
                info["outer"] = it + 1
                if _outer_converged(before[i][0], before[i][1], frames[w][-1]) or it + 1 == self.max_outer:
                    # marginalize frame 0 (:1453-1546): previous prior, IMU factor 0-1, the stored lidar factors of frame 0
                    if len(slots[w]) < 2:
                        self.priors[w] = None
                    elif on_device:
                        closing.append(i)
                    else:
                        self.priors[w] = solvers[i].marginalize(rec0[i], x)
                else:
                    still.append(w)
            if closing:                                        # one device call for every window that closes here
                pr = M.fullwindow_marginalize_batch(ctx, [solvers[i] for i in closing], [slots[active[i]][0] for i in closing],
                                                    self.T_bl, [xo[i] for i in closing])
                for i, p in zip(closing, pr):
                    self.priors[active[i]] = p
            active = still
            if not active:
                break
        return infos


def preintegrate_windows(samples, frames, ctx=None):
    """The pre-integrations of n windows from ONE mml_imu_preintegrate_batch call, in the shape BatchWindowEstimator.estimate
    takes: samples[w][f] (f >= 1; entry 0 is not read) are the IMU messages between frames f-1 and f of window w, (k, 7),
    linearised at frames[w][f-1]["bg"] / ["ba"].  Returns preints with preints[w][0] None and preints[w][f] an ImuPreint.
    ctx None: the host routine; a Context: the device call, bit-identical to it."""
    import importlib
    M = importlib.import_module(__package__)
    if len(samples) != len(frames):
        raise ValueError("samples and frames must have one entry per window (%d, %d)" % (len(samples), len(frames)))
    flat, bg, ba = [], [], []
    for w, (sw, fw) in enumerate(zip(samples, frames)):
        if len(sw) != len(fw):
            raise ValueError("window %d: samples and frames differ in length" % w)
        for f in range(1, len(fw)):
            flat.append(sw[f])
            bg.append(fw[f - 1]["bg"])
            ba.append(fw[f - 1]["ba"])
    pres = iter(M.imu_preintegrate_batch(flat, np.stack(bg), np.stack(ba), ctx) if flat else [])
    return [[None] + [next(pres) for _ in range(1, len(fw))] for fw in frames]


def fetch_imu_windows(stream_or_msgs, stamps_per_window, frames, ctx=None):
    """preintegrate_windows from raw IMU messages: fetchImuMsgs and the pre-integration of every frame interval of n windows in
    ONE imu_fetch_batch call.  stream_or_msgs: an ImuStream (the device call) or an (m, 7) array of messages (the host routine,
    bit-identical to it); stamps_per_window[w]: the stamps of window w's frames, optionally with one more in front (the stamp
    before frame 0, which then gets its messages too; otherwise samples[w][0] is empty).  Frame f's interval is
    (stamp[f-1], stamp[f]], linearised at frames[w][f-1]["bg"] / ["ba"] (frame 0: its own).  Returns (samples, preints):
    samples[w][f] a (k, 7) array, preints[w][0] None and preints[w][f] an ImuPreint -- the shapes preintegrate_windows,
    BatchWindowEstimator.estimate and try_map_initialization_batch take.  An interval that is not cut (any status but 0) raises
    ValueError naming the window, the frame and the status."""
    import importlib
    M = importlib.import_module(__package__)
    if len(stamps_per_window) != len(frames):
        raise ValueError("stamps_per_window and frames must have one entry per window (%d, %d)" % (len(stamps_per_window), len(frames)))
    ts, te, bg, ba, where = [], [], [], [], []
    for w, (sw, fw) in enumerate(zip(stamps_per_window, frames)):
        lead = len(sw) - len(fw)
        if lead not in (0, 1):
            raise ValueError("window %d: %d stamps for %d frames" % (w, len(sw), len(fw)))
        for f in range(1 - lead, len(fw)):
            ts.append(sw[f + lead - 1])
            te.append(sw[f + lead])
            bg.append(fw[max(f - 1, 0)]["bg"])
            ba.append(fw[max(f - 1, 0)]["ba"])
            where.append((w, f))
    samples = [[np.zeros((0, 7)) for _ in fw] for fw in frames]
    preints = [[None] * len(fw) for fw in frames]
    if not where:
        return samples, preints
    out = M.imu_fetch_batch(stream_or_msgs, ts, te, np.stack(bg), np.stack(ba), ctx, want=("samples", "pre"))
    o = out["offsets"]
    for i, (w, f) in enumerate(where):
        if out["rows"]["status"][i] != M.IMU_FETCH_OK:
            raise ValueError("window %d, frame %d: the interval (%r, %r] is not cut: status %d" % (w, f, ts[i], te[i], out["rows"]["status"][i]))
        samples[w][f] = out["samples"][o[i]:o[i + 1]].copy()
        if f >= 1:
            preints[w][f] = M.ImuPreint.from_buffer_copy(out["pre"][i])
    return samples, preints


def ingest_union_clouds(ctx, first_slot, messages, imu_rows=None, n_points=None, **opts):
    """The pose node's way in for a replay: the union_cloud messages of n frames (`messages`: what Context.feature_clouds
    returns, or the raw block with n_points (n, 6)) into slots first_slot .. first_slot + n - 1 with ONE Context.pose_ingest
    call, which also takes the node's decision per message (unionPoseEstimation.cpp:719-773).  imu_rows: out["rows"] of
    imu_fetch_batch for the frames' intervals, or None without an IMU.  opts: hori_rotate_th, velo_rotate_th, velo_only_mode,
    first_frame.  Returns (rows, slots): the POSE_INGEST_ROW_DTYPE rows and the slots that hold a frame (the dropped ones left
    out) -- what imu_predict_batch's dR / dt and then Context.undistort / step are to be called for; consecutive slots make one
    call."""
    import importlib
    M = importlib.import_module(__package__)
    rows = ctx.pose_ingest(first_slot, messages, n_points, imu_rows, **opts)
    slots = [first_slot + i for i in range(len(rows)) if rows["decision"][i] != M.INGEST_DROPPED]
    return rows, slots


def try_map_initialization(frames, samples, exTlb=None):
    """TryMAPInitialization (unionPoseEstimation.cpp:425-625) through mml_lio_initialize.  frames: the reference's frame
    list, front first, as dicts in the shape WindowEstimator.estimate uses (P, Q as x y z w = the lidar pose, V, bg, ba)
    plus the time stamp "t" and, for frames after the first, optionally "pre": the pre-integration the frame holds
    (without it: frame i's samples pre-integrated with frame i-1's biases).  samples: list of the frames' IMU messages
    ((k, 7) arrays as for imu_preintegrate).  Both lists are changed in place the way the reference changes its
    std::list: on success every frame gets the new V / bg / ba, frames after the first their redone "pre", the lists
    are trimmed to SLIDEWINDOWSIZE (5) and the back frame alone is moved from the lidar to the body; when the biases are
    too large nothing is written; when a velocity is too large the frames up to it keep the partial writes.
    Returns (ok, gravity, preints): preints[f] (f >= 1) between frames f-1 and f of the (trimmed) list, ready for
    WindowEstimator(gravity=gravity).estimate(slots, frames, preints)."""
    import importlib
    M = importlib.import_module(__package__)
    pre = [None] + [fr["pre"] for fr in frames[1:]] if all("pre" in fr for fr in frames[1:]) else None
    res, st, pres = M.lio_initialize([fr["t"] for fr in frames], [fr["P"] for fr in frames], [fr["Q"] for fr in frames],
                                     [fr["V"] for fr in frames], [fr["bg"] for fr in frames], [fr["ba"] for fr in frames],
                                     samples, np.eye(4) if exTlb is None else exTlb, pre)
    return _apply_map_initialization(M, frames, samples, res, st, pres)


def _apply_map_initialization(M, frames, samples, res, st, pres):
    """The list edits of TryMAPInitialization for one frame list, from what lio_initialize / lio_initialize_batch returned."""
    n = len(frames)
    gravity = np.array(res.gravity)
    if res.status in (M.LIO_INIT_BIAS, M.LIO_INIT_NOT_PD):
        return False, gravity, pres
    written = n if res.status == M.LIO_INIT_OK else res.fail_frame + 1
    for i in range(written):
        frames[i]["bg"], frames[i]["ba"] = st["bg"][i].copy(), st["ba"][i].copy()
        if res.status == M.LIO_INIT_OK or i < res.fail_frame:
            frames[i]["V"] = st["V"][i].copy()
    if res.status != M.LIO_INIT_OK:
        return False, gravity, pres
    for i in range(1, n):
        frames[i]["pre"] = pres[i]
    frames[-1]["P"], frames[-1]["Q"] = st["P"][-1].copy(), st["Q"][-1].copy()
    del frames[:res.keep_from]
    del samples[:res.keep_from]
    pres = [None] + pres[1 + res.keep_from:]
    return True, gravity, pres


def try_map_initialization_batch(frames_list, samples_list, exTlb=None, ctx=None):
    """try_map_initialization for n segments through ONE mml_lio_initialize_batch call: frames_list[s] / samples_list[s] are one
    segment's frame list and IMU messages, each changed in place exactly as try_map_initialization changes them; exTlb: None
    (identity), one 4 x 4 for all, or one per segment (n, 4, 4).  A segment whose pre-integration covariance is not positive
    definite (status LIO_INIT_NOT_PD, e.g. an empty interval) counts as not ok with nothing written.  ctx None: the host
    routine; a Context: the device call, bit-identical to it.  Returns a list of (ok, gravity, preints), ready for
    BatchWindowEstimator(gravity=np.stack([g for _, g, _ in out]))."""
    import importlib
    M = importlib.import_module(__package__)
    n_seg = len(frames_list)
    if len(samples_list) != n_seg:
        raise ValueError("frames_list and samples_list must have one entry per segment (%d, %d)" % (n_seg, len(samples_list)))
    ex = np.eye(4) if exTlb is None else np.asarray(exTlb, dtype=np.float64)
    if ex.shape not in ((4, 4), (n_seg, 4, 4)):
        raise ValueError("exTlb must be one 4 x 4 matrix or one per segment (%d, 4, 4), not %s" % (n_seg, ex.shape))
    ex = np.broadcast_to(ex, (n_seg, 4, 4))
    segs = []
    for s, frames in enumerate(frames_list):
        pre = [None] + [fr["pre"] for fr in frames[1:]] if all("pre" in fr for fr in frames[1:]) else None
        segs.append(([fr["t"] for fr in frames], [fr["P"] for fr in frames], [fr["Q"] for fr in frames], [fr["V"] for fr in frames],
                     [fr["bg"] for fr in frames], [fr["ba"] for fr in frames], samples_list[s], ex[s], pre))
    out = M.lio_initialize_batch(segs, ctx)
    return [_apply_map_initialization(M, frames_list[s], samples_list[s], *out[s]) for s in range(n_seg)]


def time_offset_from_frames(ctx, velo_frames, livox, tf=None, search_resolution=30, sliced_points=12000):
    """The aligner's time-offset estimate from raw Velodyne frames: velo_cloud_handler's FOV selection
    (unionLidarsAligner.cpp:437-490) of every frame in one device call, then estimate_timeoffset's search (:1077-1153) of every
    selected cloud in one more.  velo_frames: list of (n_i, k >= 3) float32 rows x, y, z, ...; livox: one merged Livox cloud (m, 3)
    searched by every frame, or one per frame; tf: None, one 4 x 4 matrix or one per frame (_velo_hori_tf_matrix).  The selection's
    packed x, y, z rows and the running sums of its counts go into the search as they are.  Returns (results, selection): the
    list of dicts Context.time_offset_search_batch returns and the dict of Context.velo_fov_select."""
    sel = ctx.velo_fov_select(velo_frames)
    n = len(sel["n_kept"])
    vo = sel["offsets"]
    if isinstance(livox, np.ndarray) or (len(livox) and np.ndim(livox[0]) == 1):
        livox = [livox] * n
    if len(livox) != n:
        raise ValueError("%d Livox clouds for %d Velodyne frames" % (len(livox), n))
    velo_list = [sel["xyz"][vo[i]:vo[i + 1]] for i in range(n)]     # (views: time_offset_pack concatenates them back in order)
    return ctx.time_offset_search_batch(velo_list, livox, search_resolution, sliced_points, tfs=tf), sel


def time_offset_from_stream(ctx, stream, message_marks, velo_frames, velo_stamps, hori_stamp, tf=None, search_resolution=30,
                            sliced_points=12000, error_th=1e6, all_frames=False):
    """LidarsParamEstimator::estimate_timeoffset (unionLidarsAligner.cpp:1021-1166) on a resident Livox stream: the gate of
    :1026-1043 (time_offset_gate), then ONE Context.time_offset_estimate_stream call for the frame it selects against the merged
    last eight messages (:1049-1074).  message_marks: per pushed message its first point's absolute index, in push order, with the
    stream's tail as one more entry (len = messages + 1) -- what the caller knows from its pushes; velo_frames / velo_stamps: the
    queued Velodyne frames, oldest first, and their header stamps (ns); hori_stamp: the newest Livox message's header stamp.
    Returns (row, selected, status): the selected frame's dict (None when the gate refuses: TOFS_GATE_EMPTY,
    TOFS_GATE_TOO_FEW_MESSAGES), its index and the gate's status.  all_frames=True runs every queued frame in the one call and
    returns the list of their dicts in the place of row (the gate's answer still comes with it; None only for too few messages)."""
    import importlib
    M = importlib.import_module(__package__)
    marks = [int(m) for m in message_marks]
    n_msgs = len(marks) - 1
    selected, status = M.time_offset_gate(velo_stamps, hori_stamp, n_msgs)
    if n_msgs < 8 or (selected < 0 and not all_frames):
        return None, selected, status
    begin, end = marks[n_msgs - 8], marks[n_msgs]
    which = list(range(len(velo_frames))) if all_frames else [selected]
    rows = ctx.time_offset_estimate_stream(stream, begin, end, [velo_frames[i] for i in which], [int(velo_stamps[i]) for i in which], tf,
                                           search_resolution, sliced_points, error_th)
    return (rows if all_frames else rows[0]), selected, status
