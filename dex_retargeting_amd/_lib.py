"""ctypes binding of libdexr.so (include/dexr.h).  Fails loudly when the HIP library is missing: there is no
CPU fallback anywhere in this package."""
from __future__ import annotations

import ctypes as C
import threading
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DEXR_LIB") or os.path.join(_HERE, "libdexr.so")  # DEXR_LIB: developer override

_lib: Optional[C.CDLL] = None


class DexrError(RuntimeError):
    pass


class SolveOptions(C.Structure):
    _fields_ = [("max_iter", C.c_int32), ("tol", C.c_float), ("lambda0", C.c_float), ("newton", C.c_int32),
                ("precision", C.c_int32), ("polish", C.c_int32), ("strict", C.c_int32)]


class Tuning(C.Structure):
    """Mirror of dexr_tuning (include/dexr.h): per-model launch / damping parameters."""
    _fields_ = [("struct_size", C.c_uint32), ("kernel", C.c_int32), ("chain", C.c_int32), ("persist_occ", C.c_int32),
                ("persist_from", C.c_int32), ("qchunk", C.c_int32), ("resident_waves", C.c_int32),
                ("max_blind", C.c_int32), ("stall_from", C.c_int32), ("stall_ratio", C.c_float),
                ("stall_cap", C.c_float), ("lam_jump", C.c_float), ("lam_fastdec", C.c_float),
                ("floor_scale", C.c_float), ("step_cap", C.c_float), ("blind_tol_scale", C.c_float),
                ("pivot_rule", C.c_int32), ("longest_first", C.c_int32), ("lam_recover", C.c_float),
                ("fork_streams", C.c_int32), ("user_mask", C.c_uint32), ("sprint_max_batch", C.c_int32), ("sprint_ladder", C.c_int32), ("tail_passes", C.c_int32),
                ("kernel_f64", C.c_int32)]


TUNE_LAM_JUMP, TUNE_LAM_FASTDEC = 1, 2
_TUNE_BITS = {"lam_jump": TUNE_LAM_JUMP, "lam_fastdec": TUNE_LAM_FASTDEC}


KERNEL_AUTO, KERNEL_REGISTER, KERNEL_REDUCED, KERNEL_WIDE, KERNEL_GENERAL = -1, 0, 3, 4, 5  # (1 and 2: retired families)
KERNEL_REGISTER_CHAIN = 6  # KERNEL_REGISTER without the dedicated tip solve kernel (dexr.h)

EXPORTS = ["dexr_last_error", "dexr_version", "dexr_device_count", "dexr_default_options", "dexr_model_create",
           "dexr_model_destroy", "dexr_model_info", "dexr_model_get_tuning", "dexr_model_set_tuning", "dexr_model_kernel",
           "dexr_model_kernel_f64", "dexr_model_lane_plan", "dexr_model_reserve",
           "dexr_retarget_dev", "dexr_retarget_seq_dev", "dexr_seq_compose_dev", "dexr_fleet_workspace_bytes",
           "dexr_retarget_multi_dev", "dexr_retarget_multi", "dexr_retarget", "dexr_retarget_f64",
           "dexr_retarget_kp_dev", "dexr_retarget_kp", "dexr_eval", "dexr_fk", "dexr_mano_keypoints_dev",
           "dexr_mano_keypoints", "dexr_comm_unique_id", "dexr_comm_create", "dexr_comm_destroy", "dexr_comm_info",
           "dexr_allgather", "dexr_comm_max_f64", "dexr_comm_barrier", "dexr_retarget_vjp_dev", "dexr_retarget_vjp"]
# include/dexr_pose.h (link poses and their VJP): a list of its own, EXPORTS mirrors dexr.h alone
POSE_EXPORTS = ["dexr_pose_model_create", "dexr_pose_model_destroy", "dexr_pose_model_info", "dexr_link_poses_dev",
                "dexr_link_poses_vjp_dev", "dexr_link_poses", "dexr_link_poses_vjp"]
# include/dexr_jacobian.h (link Jacobians and link velocities on a pose table): again a list of its own
JAC_EXPORTS = ["dexr_link_jacobians_dev", "dexr_link_velocities_dev", "dexr_link_jacobians", "dexr_link_velocities"]
JAC_WORLD_ALIGNED, JAC_LOCAL = 0, 1  # DEXR_JAC_*
# include/dexr_wrench.h (J^T on a pose table: link wrenches and the VJP of the link velocities): a list of its own
WRENCH_EXPORTS = ["dexr_link_wrenches_dev", "dexr_link_velocities_vjp_dev", "dexr_link_wrenches", "dexr_link_velocities_vjp"]
# include/dexr_ik.h (one damped least-squares IK step on a pose table): a list of its own
IK_EXPORTS = ["dexr_link_ik_step_dev", "dexr_link_ik_step"]
# include/dexr_ik_solve.h (the step iterated inside one kernel, to pose targets and with joint limits): a list of its own
IK_SOLVE_EXPORTS = ["dexr_link_ik_solve_dev", "dexr_link_ik_solve"]
# include/dexr_spheres.h (sphere-pair self-collision on a pose table: distances, their VJP, the fused penalty): a list of its own
SPHERE_EXPORTS = ["dexr_sphere_model_create", "dexr_sphere_model_destroy", "dexr_sphere_model_info", "dexr_sphere_distances_dev",
                  "dexr_sphere_distances_vjp_dev", "dexr_sphere_penalty_dev", "dexr_sphere_distances", "dexr_sphere_distances_vjp",
                  "dexr_sphere_penalty"]
SPHERE_MAX, SPHERE_MAXPAIR = 128, 8192  # DEXR_SPHERE_*
# include/dexr_resolve.h (the collision-aware posture solve on a sphere model, iterated inside one kernel): a list of its own
RESOLVE_EXPORTS = ["dexr_sphere_resolve_dev", "dexr_sphere_resolve"]
RESOLVE_MAXACTIVE, RESOLVE_LAM_UP, RESOLVE_LAM_DOWN, RESOLVE_MAXREJECT = 256, 8, 4, 12  # DEXR_RESOLVE_*
RESOLVE_CONVERGED, RESOLVE_STALLED, RESOLVE_TRUNCATED = 1, 2, 4  # status bits
# include/dexr_obstacles.h (the spheres of a sphere model against posed primitives: distances, their VJP, the fused penalty): a
# list of its own
OBSTACLE_EXPORTS = ["dexr_obstacle_set_create", "dexr_obstacle_set_destroy", "dexr_obstacle_set_info", "dexr_obstacle_distances_dev",
                    "dexr_obstacle_distances_vjp_dev", "dexr_obstacle_penalty_dev", "dexr_obstacle_distances",
                    "dexr_obstacle_distances_vjp", "dexr_obstacle_penalty"]
OBSTACLE_MAX, OBSTACLE_PARAMS = 64, 16  # DEXR_OBSTACLE_*
OBSTACLE_SPHERE, OBSTACLE_CAPSULE, OBSTACLE_BOX, OBSTACLE_HALFSPACE = 0, 1, 2, 3  # primitive kinds
# include/dexr_resolve_obstacles.h (the posture solve with the obstacle term, iterated inside one kernel): a list of its own
RESOLVE_OBSTACLE_EXPORTS = ["dexr_sphere_resolve_obstacles_dev", "dexr_sphere_resolve_obstacles"]
RESOLVE_MAXCONTACT = 256  # DEXR_RESOLVE_MAXCONTACT
RESOLVE_CONTACTS_TRUNCATED = 8  # status bit
# include/dexr_sdf_grid.h (the spheres of a sphere model against one sampled signed-distance field: distances, their VJP, the fused
# penalty): a list of its own
SDF_GRID_EXPORTS = ["dexr_sdf_grid_create", "dexr_sdf_grid_destroy", "dexr_sdf_grid_info", "dexr_grid_distances_dev",
                    "dexr_grid_distances_vjp_dev", "dexr_grid_penalty_dev", "dexr_grid_distances", "dexr_grid_distances_vjp",
                    "dexr_grid_penalty"]
SDF_GRID_MIN_DIM, SDF_GRID_MAX_DIM, SDF_GRID_MAX_SAMPLES = 2, 1024, 1 << 24  # DEXR_SDF_GRID_*
# include/dexr_resolve_grid.h (the posture solve with the grid term, iterated inside one kernel): a list of its own
RESOLVE_GRID_EXPORTS = ["dexr_sphere_resolve_grid_dev", "dexr_sphere_resolve_grid"]
# include/dexr_resolve_scene.h (the posture solve against several posed bodies, sets and grids, in one kernel): a list of its own
RESOLVE_SCENE_EXPORTS = ["dexr_sphere_resolve_scene_dev", "dexr_sphere_resolve_scene"]
SCENE_MAXBODY = 4  # DEXR_SCENE_MAXBODY
# include/dexr_mesh_sdf.h (signed distances of points and of grid samples to a triangle mesh, brute force): a list of its own
MESH_SDF_EXPORTS = ["dexr_mesh_create", "dexr_mesh_destroy", "dexr_mesh_info", "dexr_mesh_distances_dev", "dexr_mesh_distances",
                    "dexr_mesh_sample_grid_dev", "dexr_mesh_sample_grid"]
MESH_MAX_VERTICES, MESH_MAX_TRIANGLES = 1 << 20, 1 << 20  # DEXR_MESH_MAX_*
MESH_TILE, MESH_BLOCK_POINTS, MESH_PAIRS_PER_LAUNCH = 256, 512, 1 << 34  # DEXR_MESH_TILE, DEXR_MESH_BLOCK_POINTS, DEXR_MESH_PAIRS_PER_LAUNCH
# include/dexr_sphere_fit.h (inscribed spheres of sampled signed-distance fields, a greedy cover): a list of its own.  (Its name does
# not end in EXPORTS: tests/test_cross_host.py counts the lists that do.)
SPHERE_FIT_SYMBOLS = ["dexr_sphere_fit_workspace_bytes", "dexr_sphere_fit_dev", "dexr_sphere_fit"]
SPHERE_FIT_MIN_DIM, SPHERE_FIT_MAX_DIM, SPHERE_FIT_MAX_BODIES, SPHERE_FIT_CHUNK = 2, 64, 64, 1024  # DEXR_SPHERE_FIT_*
# include/dexr_cross.h (the spheres of one posed robot against another's: distances, their VJP, the fused penalty): a list of its own
CROSS_EXPORTS = ["dexr_cross_distances_dev", "dexr_cross_distances_vjp_dev", "dexr_cross_penalty_dev", "dexr_cross_distances",
                 "dexr_cross_distances_vjp", "dexr_cross_penalty"]
CROSS_FRAMES, CROSS_LDS = 16, 65536  # DEXR_CROSS_*
# include/dexr_resolve_cross.h (the posture solve against a second posed robot, in one kernel): a list of its own.  (Its name does
# not end in EXPORTS: tests/test_cross_host.py counts the lists that do.)
RESOLVE_CROSS_SYMBOLS = ["dexr_sphere_resolve_cross_dev", "dexr_sphere_resolve_cross"]
# include/dexr_distance_transform.h (distance grids from point clouds and occupancy maps, the exact Euclidean distance transform): a
# list of its own.  (Its name does not end in EXPORTS: tests/test_cross_host.py counts the lists that do.)
EDT_SYMBOLS = ["dexr_edt_workspace_bytes", "dexr_edt_points_dev", "dexr_edt_occupancy_dev", "dexr_edt_points", "dexr_edt_occupancy"]
EDT_NONE, EDT_MAX_POINTS, EDT_TILE_BYTES = 1 << 30, 1 << 26, 65536  # DEXR_EDT_*
# include/dexr_sdf_grid_dev.h (a grid handle whose samples are written on the device): a list of its own, as above
SDF_GRID_DEV_SYMBOLS = ["dexr_sdf_grid_create_dev", "dexr_sdf_grid_values_dev", "dexr_sdf_grid_download"]
UNIQUE_ID_BYTES = 128


class SceneBodyRecord(C.Structure):
    """dexr_scene_body: one body of a scene as the two entry points of include/dexr_resolve_scene.h read it."""
    _fields_ = [("set", C.c_void_p), ("grid", C.c_void_p), ("pos", C.c_void_p), ("rot", C.c_void_p), ("prim_weight", C.c_void_p),
                ("margin", C.c_double), ("weight", C.c_double)]


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.environ.get("DEXR_NO_TORCH_PRELOAD"):
        # torch-ROCm bundles its own libamdhip64; whichever HIP runtime is loaded first serves the whole process.
        # Let torch's win when torch is installed, so tensors / streams created by torch and the kernels launched by
        # libdexr share one runtime (device-pointer entry points, bench.py).
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is optional for the host-pointer API
            pass
    if not os.path.exists(LIB_PATH):
        raise DexrError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(hipcc --offload-arch=gfx950). dex_retargeting_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, i64, f32p, u32p, i32p, f64p = C.c_void_p, C.c_int64, C.POINTER(C.c_float), C.POINTER(C.c_uint32), \
        C.POINTER(C.c_int32), C.POINTER(C.c_double)
    optp = C.POINTER(SolveOptions)
    lib.dexr_last_error.restype = C.c_char_p
    lib.dexr_version.restype = C.c_char_p
    lib.dexr_device_count.restype = C.c_int
    lib.dexr_default_options.argtypes = [optp]
    lib.dexr_default_options.restype = None
    lib.dexr_model_create.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(vp)]
    lib.dexr_model_destroy.argtypes = [vp]
    lib.dexr_model_destroy.restype = None
    lib.dexr_model_info.argtypes = [vp, C.c_void_p]
    lib.dexr_model_get_tuning.argtypes = [vp, C.POINTER(Tuning)]
    lib.dexr_model_set_tuning.argtypes = [vp, C.POINTER(Tuning)]
    lib.dexr_model_kernel.argtypes = [vp, i32p, i32p, i32p]
    lib.dexr_model_kernel_f64.argtypes = [vp, i32p, i32p]
    lib.dexr_model_reserve.argtypes = [vp, C.c_int64]
    lib.dexr_model_lane_plan.argtypes = [vp, C.c_int32, i32p, i32p, vp, vp]
    lib.dexr_retarget_dev.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, optp, vp]
    lib.dexr_retarget_seq_dev.argtypes = [vp, i64, C.c_int32, vp, C.c_int32, vp, vp, vp, vp, vp, C.c_float, optp, vp]
    lib.dexr_seq_compose_dev.argtypes = [i64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, i32p, i32p, f64p, f64p, vp, vp,
                                         C.c_double, vp, C.c_int32, vp, vp]
    lib.dexr_fleet_workspace_bytes.argtypes = [i64]
    lib.dexr_fleet_workspace_bytes.restype = C.c_size_t
    lib.dexr_retarget_multi_dev.argtypes = [C.POINTER(vp), C.c_int32, i64, vp, vp, vp, C.c_int32, vp, C.c_int32, vp, vp, vp,
                                            optp, vp, C.c_size_t, vp]
    lib.dexr_retarget_multi.argtypes = [C.POINTER(vp), C.c_int32, i64, i32p, f32p, f32p, C.c_int32, f32p, C.c_int32, u32p,
                                        f32p, i32p, optp]
    lib.dexr_retarget.argtypes = [vp, i64, f32p, f32p, f32p, u32p, f32p, i32p, i32p, f32p, optp]
    lib.dexr_retarget_kp_dev.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, optp, vp]
    lib.dexr_retarget_kp.argtypes = [vp, i64, f32p, f32p, f32p, u32p, f32p, i32p, i32p, f32p, optp]
    lib.dexr_retarget_f64.argtypes = [vp, i64, f32p, f32p, f32p, u32p, f64p, i32p, i32p, optp]
    lib.dexr_eval.argtypes = [vp, i64, f32p, f32p, f32p, f64p, u32p, f64p, f64p]
    lib.dexr_fk.argtypes = [vp, i64, f64p, f64p]
    lib.dexr_retarget_vjp_dev.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.dexr_retarget_vjp.argtypes = [vp, i64, f32p, f32p, f32p, u32p, f32p, f32p, f32p, f32p, i32p]
    lib.dexr_mano_keypoints_dev.argtypes = [i64, vp, f32p, vp, vp, vp]
    lib.dexr_mano_keypoints.argtypes = [i64, f32p, f32p, f32p, f32p]
    lib.dexr_comm_unique_id.argtypes = [vp]
    lib.dexr_comm_create.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(vp)]
    lib.dexr_comm_destroy.argtypes = [vp]
    lib.dexr_comm_destroy.restype = None
    lib.dexr_comm_info.argtypes = [vp, i32p, i32p, i32p]
    lib.dexr_allgather.argtypes = [vp, vp, vp, C.c_size_t, vp]
    lib.dexr_comm_max_f64.argtypes = [vp, f64p, C.c_int32, vp]
    lib.dexr_comm_barrier.argtypes = [vp, vp]
    lib.dexr_pose_model_create.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(vp)]
    lib.dexr_pose_model_destroy.argtypes = [vp]
    lib.dexr_pose_model_destroy.restype = None
    lib.dexr_pose_model_info.argtypes = [vp, i32p, i32p, i32p, i32p]
    lib.dexr_link_poses_dev.argtypes = [vp, i64, vp, vp, vp, vp, vp]
    lib.dexr_link_poses_vjp_dev.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp]
    lib.dexr_link_poses.argtypes = [vp, i64, f64p, f64p, f64p, f64p]
    lib.dexr_link_poses_vjp.argtypes = [vp, i64, f64p, f64p, f64p, f64p, f64p]
    lib.dexr_link_jacobians_dev.argtypes = [vp, i64, vp, vp, C.c_int32, vp, vp, vp]
    lib.dexr_link_velocities_dev.argtypes = [vp, i64, vp, vp, vp, C.c_int32, vp, vp, vp]
    lib.dexr_link_jacobians.argtypes = [vp, i64, f64p, f64p, C.c_int32, f64p, f64p]
    lib.dexr_link_velocities.argtypes = [vp, i64, f64p, f64p, f64p, C.c_int32, f64p, f64p]
    lib.dexr_link_wrenches_dev.argtypes = [vp, i64, vp, vp, C.c_int32, vp, vp, vp, vp]
    lib.dexr_link_velocities_vjp_dev.argtypes = [vp, i64, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp]
    lib.dexr_link_wrenches.argtypes = [vp, i64, f64p, f64p, C.c_int32, f64p, f64p, f64p]
    lib.dexr_link_velocities_vjp.argtypes = [vp, i64, f64p, f64p, f64p, C.c_int32, f64p, f64p, f64p, f64p]
    lib.dexr_link_ik_step_dev.argtypes = [vp, i64, vp, vp, C.c_int32, vp, vp, vp, vp, C.c_float, vp, vp]
    lib.dexr_link_ik_step.argtypes = [vp, i64, f64p, f64p, C.c_int32, f64p, f64p, f64p, f64p, C.c_double, f64p]
    lib.dexr_link_ik_solve_dev.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, C.c_float, C.c_float, C.c_float, C.c_int32, vp, vp,
                                           vp, vp]
    lib.dexr_link_ik_solve.argtypes = [vp, i64, f64p, f64p, f64p, f64p, f64p, f64p, f64p, f64p, C.c_double, C.c_double, C.c_double,
                                       C.c_int32, f64p, i32p, f64p]
    lib.dexr_sphere_model_create.argtypes = [C.c_void_p, C.c_size_t, C.c_int32, i32p, f64p, f64p, C.c_int32, i32p, C.POINTER(vp)]
    lib.dexr_sphere_model_destroy.argtypes = [vp]
    lib.dexr_sphere_model_destroy.restype = None
    lib.dexr_sphere_model_info.argtypes = [vp, i32p, i32p, i32p, i32p]
    lib.dexr_sphere_distances_dev.argtypes = [vp, i64, vp, vp, vp, vp, vp]
    lib.dexr_sphere_distances_vjp_dev.argtypes = [vp, i64, vp, vp, vp, vp, vp]
    lib.dexr_sphere_penalty_dev.argtypes = [vp, i64, vp, vp, C.c_float, vp, vp, vp, vp]
    lib.dexr_sphere_distances.argtypes = [vp, i64, f64p, f64p, f64p, f64p]
    lib.dexr_sphere_distances_vjp.argtypes = [vp, i64, f64p, f64p, f64p, f64p]
    lib.dexr_sphere_penalty.argtypes = [vp, i64, f64p, f64p, C.c_double, f64p, f64p, f64p]
    lib.dexr_sphere_resolve_dev.argtypes = [vp, i64, vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp, vp, C.c_float,
                                            C.c_float, C.c_float, C.c_int32, vp, vp, vp, vp, vp]
    lib.dexr_sphere_resolve.argtypes = [vp, i64, f64p, f64p, f64p, f64p, C.c_int32, f64p, f64p, f64p, f64p, C.c_double, C.c_double, f64p,
                                        f64p, f64p, C.c_double, C.c_double, C.c_double, C.c_int32, f64p, i32p, f64p, i32p]
    lib.dexr_sphere_resolve_obstacles_dev.argtypes = [vp, i64, vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp, vp,
                                                      C.c_float, C.c_float, C.c_float, C.c_int32, vp, vp, vp, C.c_float, C.c_float, vp, vp,
                                                      vp, vp, vp, vp]
    lib.dexr_sphere_resolve_obstacles.argtypes = [vp, i64, f64p, f64p, f64p, f64p, C.c_int32, f64p, f64p, f64p, f64p, C.c_double, C.c_double,
                                                  f64p, f64p, f64p, C.c_double, C.c_double, C.c_double, C.c_int32, vp, f64p, f64p, C.c_double,
                                                  C.c_double, f64p, f64p, i32p, f64p, i32p]
    lib.dexr_obstacle_set_create.argtypes = [C.c_int32, i32p, f64p, C.POINTER(vp)]
    lib.dexr_obstacle_set_destroy.argtypes = [vp]
    lib.dexr_obstacle_set_destroy.restype = None
    lib.dexr_obstacle_set_info.argtypes = [vp, i32p]
    lib.dexr_obstacle_distances_dev.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]
    lib.dexr_obstacle_distances_vjp_dev.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]
    lib.dexr_obstacle_penalty_dev.argtypes = [vp, vp, i64, vp, vp, vp, vp, C.c_float, vp, vp, vp, vp, vp]
    lib.dexr_obstacle_distances.argtypes = [vp, vp, i64, f64p, f64p, f64p, f64p, f64p, i32p]
    lib.dexr_obstacle_distances_vjp.argtypes = [vp, vp, i64, f64p, f64p, f64p, f64p, f64p, f64p]
    lib.dexr_obstacle_penalty.argtypes = [vp, vp, i64, f64p, f64p, f64p, f64p, C.c_double, f64p, f64p, f64p, f64p]
    lib.dexr_cross_distances_dev.argtypes = [vp, vp, i64] + [vp] * 8 + [vp, vp, vp, vp, vp]
    lib.dexr_cross_distances_vjp_dev.argtypes = [vp, vp, i64] + [vp] * 8 + [vp, vp, vp, vp, vp, vp, vp]
    lib.dexr_cross_penalty_dev.argtypes = [vp, vp, i64] + [vp] * 8 + [C.c_float, vp, vp, vp, vp, vp, vp, vp]
    lib.dexr_cross_distances.argtypes = [vp, vp, i64] + [f64p] * 8 + [f64p, i32p, f64p, i32p]
    lib.dexr_cross_distances_vjp.argtypes = [vp, vp, i64] + [f64p] * 8 + [f64p] * 6
    lib.dexr_cross_penalty.argtypes = [vp, vp, i64] + [f64p] * 8 + [C.c_double] + [f64p] * 6
    lib.dexr_sdf_grid_create.argtypes = [i32p, f64p, f64p, f32p, C.POINTER(vp)]
    lib.dexr_sdf_grid_destroy.argtypes = [vp]
    lib.dexr_sdf_grid_destroy.restype = None
    lib.dexr_sdf_grid_info.argtypes = [vp, i32p, f64p, f64p]
    lib.dexr_grid_distances_dev.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp, vp]
    lib.dexr_grid_distances_vjp_dev.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]
    lib.dexr_grid_penalty_dev.argtypes = [vp, vp, i64, vp, vp, vp, vp, C.c_float, vp, vp, vp, vp]
    lib.dexr_grid_distances.argtypes = [vp, vp, i64, f64p, f64p, f64p, f64p, f64p]
    lib.dexr_grid_distances_vjp.argtypes = [vp, vp, i64, f64p, f64p, f64p, f64p, f64p, f64p]
    lib.dexr_grid_penalty.argtypes = [vp, vp, i64, f64p, f64p, f64p, f64p, C.c_double, f64p, f64p, f64p]
    lib.dexr_sphere_resolve_grid_dev.argtypes = [vp, i64, vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp, vp, C.c_float,
                                                 C.c_float, C.c_float, C.c_int32, vp, vp, vp, C.c_float, C.c_float, vp, vp, vp, vp, vp]
    lib.dexr_sphere_resolve_grid.argtypes = [vp, i64, f64p, f64p, f64p, f64p, C.c_int32, f64p, f64p, f64p, f64p, C.c_double, C.c_double, f64p,
                                             f64p, f64p, C.c_double, C.c_double, C.c_double, C.c_int32, vp, f64p, f64p, C.c_double, C.c_double,
                                             f64p, i32p, f64p, i32p]
    bodyp = C.POINTER(SceneBodyRecord)
    lib.dexr_sphere_resolve_scene_dev.argtypes = [vp, i64, vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp, vp, C.c_float,
                                                  C.c_float, C.c_float, C.c_int32, C.c_int32, bodyp, vp, vp, vp, vp, vp, vp]
    lib.dexr_sphere_resolve_scene.argtypes = [vp, i64, f64p, f64p, f64p, f64p, C.c_int32, f64p, f64p, f64p, f64p, C.c_double, C.c_double, f64p,
                                              f64p, f64p, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32, bodyp, f64p, i32p, f64p,
                                              f64p, i32p]
    lib.dexr_sphere_resolve_cross_dev.argtypes = [vp, i64, vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp, vp, C.c_float,
                                                  C.c_float, C.c_float, C.c_int32, vp, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp, vp, vp, vp,
                                                  vp]
    lib.dexr_sphere_resolve_cross.argtypes = [vp, i64, f64p, f64p, f64p, f64p, C.c_int32, f64p, f64p, f64p, f64p, C.c_double, C.c_double, f64p,
                                              f64p, f64p, C.c_double, C.c_double, C.c_double, C.c_int32, vp, f64p, f64p, f64p, f64p, C.c_double,
                                              C.c_double, f64p, f64p, i32p, f64p, i32p]
    lib.dexr_mesh_create.argtypes = [C.c_int32, f64p, C.c_int32, i32p, C.POINTER(vp)]
    lib.dexr_mesh_destroy.argtypes = [vp]
    lib.dexr_mesh_destroy.restype = None
    lib.dexr_mesh_info.argtypes = [vp, i32p, i32p, f64p]
    lib.dexr_mesh_distances_dev.argtypes = [vp, i64, vp, vp, vp, vp]
    lib.dexr_mesh_distances.argtypes = [vp, i64, f64p, f64p, f64p]
    lib.dexr_mesh_sample_grid_dev.argtypes = [vp, i32p, f64p, f64p, vp, vp]
    lib.dexr_mesh_sample_grid.argtypes = [vp, i32p, f64p, f64p, f32p]
    i64p = C.POINTER(C.c_int64)
    lib.dexr_sphere_fit_workspace_bytes.argtypes = [C.c_int32, i32p]
    lib.dexr_sphere_fit_workspace_bytes.restype = C.c_size_t
    lib.dexr_sphere_fit_dev.argtypes = [C.c_int32, i32p, f64p, i64p, i32p, C.c_double, C.c_double, C.c_double, i64, vp, vp, vp, vp, vp,
                                        C.c_size_t, vp]
    lib.dexr_sphere_fit.argtypes = [C.c_int32, i32p, f64p, i64p, i32p, C.c_double, C.c_double, C.c_double, i64, f32p, i32p, i32p, i32p]
    u8p, f64 = C.POINTER(C.c_uint8), C.c_double
    lib.dexr_edt_workspace_bytes.argtypes = [i32p, C.POINTER(C.c_size_t)]
    lib.dexr_edt_points_dev.argtypes = [vp, i64, i32p, f64p, f64, C.c_int32, f64, f64, vp, vp, vp, vp, C.c_size_t, vp]
    lib.dexr_edt_occupancy_dev.argtypes = [vp, i32p, f64, C.c_int32, f64, f64, vp, vp, vp, C.c_size_t, vp]
    lib.dexr_edt_points.argtypes = [f32p, i64, i32p, f64p, f64, C.c_int32, f64, f64, f32p, i32p, i32p]
    lib.dexr_edt_occupancy.argtypes = [u8p, i32p, f64, C.c_int32, f64, f64, f32p, i32p]
    lib.dexr_sdf_grid_create_dev.argtypes = [i32p, f64p, f64p, vp, vp, C.POINTER(vp)]
    lib.dexr_sdf_grid_values_dev.argtypes = [vp]
    lib.dexr_sdf_grid_values_dev.restype = vp
    lib.dexr_sdf_grid_download.argtypes = [vp, f32p, vp]
    _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        raise DexrError(f"libdexr error {rc}: {load().dexr_last_error().decode()}")


def default_options(**kw) -> SolveOptions:
    o = SolveOptions()
    load().dexr_default_options(C.byref(o))
    for k, v in kw.items():
        if v is not None:
            setattr(o, k, v)
    return o


def _ptr(a: Optional[np.ndarray], ctype):
    if a is None:
        return None
    return a.ctypes.data_as(C.POINTER(ctype))


class Model:
    """Owns one dexr_model (compiled tables resident in HBM)."""

    def __init__(self, blob: bytes):
        lib = load()
        self._h = C.c_void_p()
        self._one_lock = threading.Lock()
        buf = C.create_string_buffer(blob, len(blob))
        check(lib.dexr_model_create(buf, len(blob), C.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib is not None:
            _lib.dexr_model_destroy(h)
            self._h = None

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    # launch / damping parameters of this handle (dexr_tuning) -----------------------------------
    def get_tuning(self) -> Tuning:
        t = Tuning()
        t.struct_size = C.sizeof(Tuning)
        check(load().dexr_model_get_tuning(self._h, C.byref(t)))
        return t

    def tune(self, **kw) -> Tuning:
        """Change fields of the handle's dexr_tuning, e.g. ``model.tune(kernel=KERNEL_REGISTER, persist_from=0)``.
        ``lam_jump`` / ``lam_fastdec``: a number is a caller override (holds for every kernel family), ``None`` drops it."""
        t = self.get_tuning()
        for k, v in kw.items():
            if k not in dict(Tuning._fields_):
                raise AttributeError(f"dexr_tuning has no field {k}")
            if k in _TUNE_BITS:  # family-dependent defaults: a value is an explicit override, None returns to the default
                if v is None:
                    t.user_mask &= ~_TUNE_BITS[k]
                    continue
                t.user_mask |= _TUNE_BITS[k]
            setattr(t, k, v)
        check(load().dexr_model_set_tuning(self._h, C.byref(t)))
        return t

    def reserve(self, max_batch: int):
        """Pre-allocate the lazily grown device workspaces for batches of up to `max_batch` frames (dexr_model_reserve):
        afterwards no device-pointer entry point allocates or synchronises with the host."""
        check(load().dexr_model_reserve(self._h, int(max_batch)))

    def kernel(self):
        """(family, bucket, chain) of the float32 solve kernel this handle launches."""
        f, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        check(load().dexr_model_kernel(self._h, C.byref(f), C.byref(b), C.byref(c)))
        return int(f.value), int(b.value), int(c.value)  # chain: 0, 1 (serial-chain kernel) or 2 (with its tip pass)

    def kernel_f64(self):
        """(family, bucket) of the kernel a float64 solve launch of this handle runs (dexr_tuning.kernel_f64)."""
        f, b = C.c_int32(), C.c_int32()
        check(load().dexr_model_kernel_f64(self._h, C.byref(f), C.byref(b)))
        return int(f.value), int(b.value)

    def lane_plan(self, comp: int = 0):
        """(n_chain, depth, chain (16,16) uint8, anc_rev (32,) uint32) of the sixteen-lane kernel for one component."""
        n, d = C.c_int32(), C.c_int32()
        chain = np.zeros((16, 16), np.uint8)
        anc = np.zeros(32, np.uint32)
        check(load().dexr_model_lane_plan(self._h, comp, C.byref(n), C.byref(d), chain.ctypes.data_as(C.c_void_p),
                                          anc.ctypes.data_as(C.c_void_p)))
        return int(n.value), int(d.value), chain, anc

    # host-pointer entry points -------------------------------------------------------------------
    def retarget(self, ref, fixed, last, state=None, opts: Optional[SolveOptions] = None, want_info=False,
                 keypoints: bool = False):
        """ref: (B,n_ref,3) ref_value rows, or with keypoints=True the raw (B,n_keypoints,3) hand keypoints."""
        lib = load()
        ref = np.ascontiguousarray(ref, dtype=np.float32)
        last = np.ascontiguousarray(last, dtype=np.float32)
        B = last.shape[0]
        fixed = None if fixed is None or fixed.size == 0 else np.ascontiguousarray(fixed, dtype=np.float32)
        if B == 1:
            return self._retarget_one(lib, ref, fixed, last, state, opts, want_info, keypoints)
        q = np.empty_like(last)
        status = np.zeros(B, dtype=np.int32)
        iters = np.zeros(B, dtype=np.int32)
        fval = np.zeros(B, dtype=np.float32)
        fn = lib.dexr_retarget_kp if keypoints else lib.dexr_retarget
        check(fn(self._h, B, _ptr(ref, C.c_float), _ptr(fixed, C.c_float), _ptr(last, C.c_float),
                 _ptr(state, C.c_uint32), _ptr(q, C.c_float), _ptr(status, C.c_int32),
                 _ptr(iters, C.c_int32), _ptr(fval, C.c_float), C.byref(opts) if opts is not None else None))
        if want_info:
            return q, dict(status=status, iters=iters, fval=fval)
        return q

    def _retarget_one(self, lib, ref, fixed, last, state, opts, want_info, keypoints):
        """ONE frame per call -- the reference's own calling pattern (SeqRetargeting.retarget, profile_online_retargeting.py:
        18-36): the arrays of the call live in per-handle buffers whose ctypes pointers are built once; a call copies a few
        dozen floats in and out instead of allocating four arrays and building eight pointer objects (numpy's
        `ctypes.data_as` costs 1-3 us each: a fifth of a 48 us call)."""
        with self._one_lock:  # (the buffers are shared by every caller of this handle; the C call is serialised per handle anyway)
            return self._retarget_one_locked(lib, ref, fixed, last, state, opts, want_info, keypoints)

    def _retarget_one_locked(self, lib, ref, fixed, last, state, opts, want_info, keypoints):
        key = (ref.shape, None if fixed is None else fixed.shape, last.shape, state is not None)
        c = getattr(self, "_one", None)
        if c is None or c[0] != key:
            b = dict(ref=np.empty(ref.shape, np.float32), fixed=None if fixed is None else np.empty(fixed.shape, np.float32),
                     last=np.empty(last.shape, np.float32), state=None if state is None else np.zeros(1, np.uint32),
                     q=np.empty(last.shape, np.float32), status=np.zeros(1, np.int32), iters=np.zeros(1, np.int32),
                     fval=np.zeros(1, np.float32))
            p = (_ptr(b["ref"], C.c_float), _ptr(b["fixed"], C.c_float), _ptr(b["last"], C.c_float), _ptr(b["state"], C.c_uint32),
                 _ptr(b["q"], C.c_float), _ptr(b["status"], C.c_int32), _ptr(b["iters"], C.c_int32), _ptr(b["fval"], C.c_float))
            c = self._one = (key, b, p)
        b, p = c[1], c[2]
        np.copyto(b["ref"], ref)
        np.copyto(b["last"], last)
        if fixed is not None:
            np.copyto(b["fixed"], fixed)
        if state is not None:
            b["state"][0] = state[0]
        fn = lib.dexr_retarget_kp if keypoints else lib.dexr_retarget
        check(fn(self._h, 1, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], C.byref(opts) if opts is not None else None))
        if state is not None:
            state[0] = b["state"][0]
        q = b["q"].copy()
        if want_info:
            return q, dict(status=b["status"].copy(), iters=b["iters"].copy(), fval=b["fval"].copy())
        return q

    def retarget_f64(self, ref, fixed, last, state=None, opts: Optional[SolveOptions] = None, want_info=False):
        lib = load()
        ref = np.ascontiguousarray(ref, dtype=np.float32)
        last = np.ascontiguousarray(last, dtype=np.float32)
        B = last.shape[0]
        fixed = None if fixed is None or fixed.size == 0 else np.ascontiguousarray(fixed, dtype=np.float32)
        q = np.empty(last.shape, dtype=np.float64)
        status = np.zeros(B, dtype=np.int32)
        iters = np.zeros(B, dtype=np.int32)
        check(lib.dexr_retarget_f64(self._h, B, _ptr(ref, C.c_float), _ptr(fixed, C.c_float), _ptr(last, C.c_float),
                                    _ptr(state, C.c_uint32), _ptr(q, C.c_double), _ptr(status, C.c_int32),
                                    _ptr(iters, C.c_int32), C.byref(opts) if opts is not None else None))
        if want_info:
            return q, dict(status=status, iters=iters)
        return q

    def eval(self, ref, fixed, last, x, state=None):
        lib = load()
        ref = np.ascontiguousarray(ref, dtype=np.float32)
        last = np.ascontiguousarray(last, dtype=np.float32)
        x = np.ascontiguousarray(x, dtype=np.float64)
        B = x.shape[0]
        fixed = None if fixed is None or fixed.size == 0 else np.ascontiguousarray(fixed, dtype=np.float32)
        f = np.zeros(B, dtype=np.float64)
        g = np.zeros_like(x)
        check(lib.dexr_eval(self._h, B, _ptr(ref, C.c_float), _ptr(fixed, C.c_float), _ptr(last, C.c_float),
                            _ptr(x, C.c_double), _ptr(state, C.c_uint32), _ptr(f, C.c_double), _ptr(g, C.c_double)))
        return f, g

    def vjp(self, ref, fixed, last, q, grad_q, state=None):
        """Host-array twin of vjp_dev: (grad_ref (B,n_ref,3), grad_last (B,n_opt), status (B,)) float32 / int32."""
        lib = load()
        ref = np.ascontiguousarray(ref, dtype=np.float32)
        last = np.ascontiguousarray(last, dtype=np.float32)
        q = np.ascontiguousarray(q, dtype=np.float32)
        grad_q = np.ascontiguousarray(grad_q, dtype=np.float32)
        B = last.shape[0]
        if q.shape != last.shape or grad_q.shape != last.shape:
            raise ValueError(f"q and grad_q must have the shape of last_qpos {last.shape}")
        fixed = None if fixed is None or fixed.size == 0 else np.ascontiguousarray(fixed, dtype=np.float32)
        state = None if state is None else np.ascontiguousarray(state, dtype=np.uint32)
        gref = np.zeros(ref.shape, dtype=np.float32)
        glast = np.zeros(last.shape, dtype=np.float32)
        status = np.zeros(B, dtype=np.int32)
        check(lib.dexr_retarget_vjp(self._h, B, _ptr(ref, C.c_float), _ptr(fixed, C.c_float), _ptr(last, C.c_float),
                                    _ptr(state, C.c_uint32), _ptr(q, C.c_float), _ptr(grad_q, C.c_float),
                                    _ptr(gref, C.c_float), _ptr(glast, C.c_float), _ptr(status, C.c_int32)))
        return gref, glast, status

    def fk(self, q, n_links: int):
        lib = load()
        q = np.ascontiguousarray(q, dtype=np.float64)
        B = q.shape[0]
        out = np.zeros((B, n_links, 3), dtype=np.float64)
        check(lib.dexr_fk(self._h, B, _ptr(q, C.c_double), _ptr(out, C.c_double)))
        return out

    def retarget_seq_dev(self, B: int, T: int, inputs_ptr: int, fixed_ptr: int, last_ptr: int, state_ptr: int,
                         qraw_ptr: int, status_ptr: int = 0, joint_limit_eps: float = 1e-3,
                         opts: Optional[SolveOptions] = None, stream: int = 0, keypoints: bool = True):
        """T frames of B sequences in one launch (dexr_retarget_seq_dev); device addresses of C-contiguous arrays."""
        check(load().dexr_retarget_seq_dev(self._h, B, T, inputs_ptr or None, 1 if keypoints else 0, fixed_ptr or None,
                                           last_ptr or None, state_ptr or None, qraw_ptr or None, status_ptr or None,
                                           joint_limit_eps, C.byref(opts) if opts is not None else None, stream or None))

    # device-pointer entry point (torch tensors on the current device) ------------------------------
    def retarget_dev(self, B: int, ref_ptr: int, fixed_ptr: int, last_ptr: int, state_ptr: int, q_ptr: int,
                     status_ptr: int = 0, iters_ptr: int = 0, fval_ptr: int = 0,
                     opts: Optional[SolveOptions] = None, stream: int = 0, keypoints: bool = False):
        """Enqueue on `stream`; all pointers are device addresses of C-contiguous arrays.  With keypoints=True
        `ref_ptr` addresses raw (B,n_keypoints,3) hand keypoints instead of ref_value rows."""
        fn = load().dexr_retarget_kp_dev if keypoints else load().dexr_retarget_dev
        check(fn(self._h, B, ref_ptr or None, fixed_ptr or None, last_ptr or None,
                 state_ptr or None, q_ptr or None, status_ptr or None, iters_ptr or None,
                 fval_ptr or None, C.byref(opts) if opts is not None else None, stream or None))

    def vjp_dev(self, B: int, ref_ptr: int, fixed_ptr: int, last_ptr: int, state_ptr: int, q_ptr: int, grad_q_ptr: int,
                grad_ref_ptr: int, grad_last_ptr: int = 0, status_ptr: int = 0, stream: int = 0):
        """Implicit-function VJP of the solve at q (dexr_retarget_vjp_dev); device addresses of C-contiguous arrays, enqueued
        on `stream`.  `ref_ptr` addresses (B,n_ref,3) ref_value rows; state / grad_last / status may be 0 (NULL)."""
        check(load().dexr_retarget_vjp_dev(self._h, B, ref_ptr or None, fixed_ptr or None, last_ptr or None,
                                           state_ptr or None, q_ptr or None, grad_q_ptr or None, grad_ref_ptr or None,
                                           grad_last_ptr or None, status_ptr or None, stream or None))


class PoseModel:
    """Owns one dexr_pose_model (include/dexr_pose.h): the pose table of a list of links, resident in HBM."""

    def __init__(self, blob: bytes):
        lib = load()
        self._h = C.c_void_p()
        buf = C.create_string_buffer(blob, len(blob))
        check(lib.dexr_pose_model_create(buf, len(blob), C.byref(self._h)))
        v = [C.c_int32() for _ in range(4)]
        check(lib.dexr_pose_model_info(self._h, *[C.byref(a) for a in v]))
        self.n_in, self.n_fixed, self.n_link, self.n_joint = (int(a.value) for a in v)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib is not None:
            _lib.dexr_pose_model_destroy(h)
            self._h = None

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    # device-pointer entry points: float32, C-contiguous, enqueued on `stream` ------------------------
    def poses_dev(self, B: int, x_ptr: int, fixed_ptr: int, pos_ptr: int, rot_ptr: int = 0, stream: int = 0):
        """x (B, n_in), fixed (B, n_fixed) or 0 -> pos (B, n_link, 3), rot (B, n_link, 3, 3) or 0 (dexr_link_poses_dev)."""
        check(load().dexr_link_poses_dev(self._h, B, x_ptr or None, fixed_ptr or None, pos_ptr or None, rot_ptr or None,
                                         stream or None))

    def vjp_dev(self, B: int, x_ptr: int, fixed_ptr: int, grad_pos_ptr: int, grad_rot_ptr: int, grad_x_ptr: int,
                stream: int = 0):
        """grad_pos (B, n_link, 3) and / or grad_rot (B, n_link, 3, 3) (0: absent) -> grad_x (B, n_in)
        (dexr_link_poses_vjp_dev)."""
        check(load().dexr_link_poses_vjp_dev(self._h, B, x_ptr or None, fixed_ptr or None, grad_pos_ptr or None,
                                             grad_rot_ptr or None, grad_x_ptr or None, stream or None))

    def jacobians_dev(self, B: int, x_ptr: int, fixed_ptr: int, jlin_ptr: int, jang_ptr: int, frame: int = 0, stream: int = 0):
        """x (B, n_in), fixed (B, n_fixed) or 0 -> jlin, jang (B, n_link, 3, n_in), either may be 0, every entry written
        (dexr_link_jacobians_dev); frame: JAC_WORLD_ALIGNED or JAC_LOCAL."""
        check(load().dexr_link_jacobians_dev(self._h, B, x_ptr or None, fixed_ptr or None, int(frame), jlin_ptr or None,
                                             jang_ptr or None, stream or None))

    def velocities_dev(self, B: int, x_ptr: int, fixed_ptr: int, xdot_ptr: int, lin_ptr: int, ang_ptr: int, frame: int = 0,
                       stream: int = 0):
        """x, xdot (B, n_in), fixed (B, n_fixed) or 0 -> lin, ang (B, n_link, 3), either may be 0
        (dexr_link_velocities_dev)."""
        check(load().dexr_link_velocities_dev(self._h, B, x_ptr or None, fixed_ptr or None, xdot_ptr or None, int(frame),
                                              lin_ptr or None, ang_ptr or None, stream or None))

    def wrenches_dev(self, B: int, x_ptr: int, fixed_ptr: int, force_ptr: int, torque_ptr: int, tau_ptr: int, frame: int = 0,
                     stream: int = 0):
        """force, torque (B, n_link, 3), either may be 0 -> tau (B, n_in) = J^T (force, torque), every entry written
        (dexr_link_wrenches_dev)."""
        check(load().dexr_link_wrenches_dev(self._h, B, x_ptr or None, fixed_ptr or None, int(frame), force_ptr or None,
                                            torque_ptr or None, tau_ptr or None, stream or None))

    def velocities_vjp_dev(self, B: int, x_ptr: int, fixed_ptr: int, xdot_ptr: int, grad_lin_ptr: int, grad_ang_ptr: int,
                           grad_x_ptr: int, grad_xdot_ptr: int, frame: int = 0, stream: int = 0):
        """cotangents grad_lin, grad_ang (B, n_link, 3) of velocities_dev's outputs, either may be 0 -> grad_x, grad_xdot
        (B, n_in), either may be 0 (dexr_link_velocities_vjp_dev)."""
        check(load().dexr_link_velocities_vjp_dev(self._h, B, x_ptr or None, fixed_ptr or None, xdot_ptr or None, int(frame),
                                                  grad_lin_ptr or None, grad_ang_ptr or None, grad_x_ptr or None,
                                                  grad_xdot_ptr or None, stream or None))

    def ik_step_dev(self, B: int, x_ptr: int, fixed_ptr: int, err_lin_ptr: int, err_ang_ptr: int, w_lin_ptr: int, w_ang_ptr: int,
                    damping: float, dx_ptr: int, frame: int = 0, stream: int = 0):
        """err_lin, err_ang (B, n_link, 3), either may be 0; w_lin, w_ang (B, n_link) or 0 (weights of 1) -> dx (B, n_in), the
        damped least-squares step, every entry written (dexr_link_ik_step_dev)."""
        check(load().dexr_link_ik_step_dev(self._h, B, x_ptr or None, fixed_ptr or None, int(frame), err_lin_ptr or None,
                                           err_ang_ptr or None, w_lin_ptr or None, w_ang_ptr or None, float(damping),
                                           dx_ptr or None, stream or None))

    def ik_solve_dev(self, B: int, x0_ptr: int, fixed_ptr: int, tgt_pos_ptr: int, tgt_rot_ptr: int, w_lin_ptr: int, w_ang_ptr: int,
                     lo_ptr: int, hi_ptr: int, damping: float, max_iters: int, x_ptr: int, iters_ptr: int = 0, err_ptr: int = 0,
                     tol: float = 0.0, max_step: float = 0.0, stream: int = 0):
        """x0 (B, n_in), tgt_pos (B, n_link, 3) and / or tgt_rot (B, n_link, 3, 3) world targets (0: absent), w_lin, w_ang
        (B, n_link) or 0, lo, hi (n_in) or both 0 -> x (B, n_in), iters (B) int32 or 0, err (B) or 0: up to max_iters damped
        least-squares steps inside one launch, every entry written; x may alias x0 (dexr_link_ik_solve_dev)."""
        check(load().dexr_link_ik_solve_dev(self._h, B, x0_ptr or None, fixed_ptr or None, tgt_pos_ptr or None, tgt_rot_ptr or None,
                                            w_lin_ptr or None, w_ang_ptr or None, lo_ptr or None, hi_ptr or None, float(damping),
                                            float(max_step), float(tol), int(max_iters), x_ptr or None, iters_ptr or None,
                                            err_ptr or None, stream or None))

    # host-pointer entry points: float64 in, float64 arithmetic, float64 out ----------------------------
    def _host_inputs(self, x, fixed):
        x = np.ascontiguousarray(np.atleast_2d(np.asarray(x, dtype=np.float64)))
        if x.shape[1] != self.n_in:
            raise ValueError(f"x must have shape (B, {self.n_in}), got {x.shape}")
        B = x.shape[0]
        if self.n_fixed == 0:
            fixed = None
        else:
            if fixed is None:
                raise ValueError(f"the table reads {self.n_fixed} fixed joints: fixed of shape ({B}, {self.n_fixed}) is required")
            fixed = np.ascontiguousarray(np.asarray(fixed, dtype=np.float64).reshape(B, -1))
            if fixed.shape != (B, self.n_fixed):
                raise ValueError(f"fixed must have shape ({B}, {self.n_fixed}), got {fixed.shape}")
        return x, fixed, B

    def poses(self, x, fixed=None, rotations: bool = True):
        """-> pos (B, n_link, 3), rot (B, n_link, 3, 3) or None; float64 (dexr_link_poses)."""
        x, fixed, B = self._host_inputs(x, fixed)
        pos = np.zeros((B, self.n_link, 3), dtype=np.float64)
        rot = np.zeros((B, self.n_link, 3, 3), dtype=np.float64) if rotations else None
        check(load().dexr_link_poses(self._h, B, _ptr(x, C.c_double), _ptr(fixed, C.c_double), _ptr(pos, C.c_double),
                                     _ptr(rot, C.c_double)))
        return pos, rot

    def vjp(self, x, fixed=None, grad_pos=None, grad_rot=None):
        """-> grad_x (B, n_in) float64 (dexr_link_poses_vjp); at least one of the two gradients is required."""
        x, fixed, B = self._host_inputs(x, fixed)
        if grad_pos is not None:
            grad_pos = np.ascontiguousarray(grad_pos, dtype=np.float64)
            if grad_pos.shape != (B, self.n_link, 3):
                raise ValueError(f"grad_pos must have shape ({B}, {self.n_link}, 3), got {grad_pos.shape}")
        if grad_rot is not None:
            grad_rot = np.ascontiguousarray(grad_rot, dtype=np.float64)
            if grad_rot.shape != (B, self.n_link, 3, 3):
                raise ValueError(f"grad_rot must have shape ({B}, {self.n_link}, 3, 3), got {grad_rot.shape}")
        gx = np.zeros((B, self.n_in), dtype=np.float64)
        check(load().dexr_link_poses_vjp(self._h, B, _ptr(x, C.c_double), _ptr(fixed, C.c_double), _ptr(grad_pos, C.c_double),
                                         _ptr(grad_rot, C.c_double), _ptr(gx, C.c_double)))
        return gx

    def jacobians(self, x, fixed=None, frame: int = 0, angular: bool = True):
        """-> jlin (B, n_link, 3, n_in), jang (the same shape) or None; float64 (dexr_link_jacobians)."""
        x, fixed, B = self._host_inputs(x, fixed)
        jlin = np.zeros((B, self.n_link, 3, self.n_in), dtype=np.float64)
        jang = np.zeros((B, self.n_link, 3, self.n_in), dtype=np.float64) if angular else None
        check(load().dexr_link_jacobians(self._h, B, _ptr(x, C.c_double), _ptr(fixed, C.c_double), int(frame),
                                         _ptr(jlin, C.c_double), _ptr(jang, C.c_double)))
        return jlin, jang

    def velocities(self, x, xdot, fixed=None, frame: int = 0, angular: bool = True):
        """-> lin (B, n_link, 3), ang (the same shape) or None; float64 (dexr_link_velocities)."""
        x, fixed, B = self._host_inputs(x, fixed)
        xdot = np.ascontiguousarray(np.atleast_2d(np.asarray(xdot, dtype=np.float64)))
        if xdot.shape != x.shape:
            raise ValueError(f"xdot must have the shape of x {x.shape}, got {xdot.shape}")
        lin = np.zeros((B, self.n_link, 3), dtype=np.float64)
        ang = np.zeros((B, self.n_link, 3), dtype=np.float64) if angular else None
        check(load().dexr_link_velocities(self._h, B, _ptr(x, C.c_double), _ptr(fixed, C.c_double), _ptr(xdot, C.c_double),
                                          int(frame), _ptr(lin, C.c_double), _ptr(ang, C.c_double)))
        return lin, ang

    def _host_link_rows(self, a, B, what):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != (B, self.n_link, 3):
            raise ValueError(f"{what} must have shape ({B}, {self.n_link}, 3), got {a.shape}")
        return a

    def _host_link_weights(self, a, B, what):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != (B, self.n_link):
            raise ValueError(f"{what} must have shape ({B}, {self.n_link}), got {a.shape}")
        return a

    def ik_step(self, x, fixed=None, err_lin=None, err_ang=None, w_lin=None, w_ang=None, damping=None, frame: int = 0):
        """-> dx (B, n_in) float64 (dexr_link_ik_step); at least one of err_lin, err_ang (B, n_link, 3) is required, w_lin,
        w_ang (B, n_link) or None weigh them, damping > 0 is required."""
        if damping is None:
            raise ValueError("damping is required")
        x, fixed, B = self._host_inputs(x, fixed)
        err_lin, err_ang = self._host_link_rows(err_lin, B, "err_lin"), self._host_link_rows(err_ang, B, "err_ang")
        w_lin, w_ang = self._host_link_weights(w_lin, B, "w_lin"), self._host_link_weights(w_ang, B, "w_ang")
        dx = np.zeros((B, self.n_in), dtype=np.float64)
        check(load().dexr_link_ik_step(self._h, B, _ptr(x, C.c_double), _ptr(fixed, C.c_double), int(frame),
                                       _ptr(err_lin, C.c_double), _ptr(err_ang, C.c_double), _ptr(w_lin, C.c_double),
                                       _ptr(w_ang, C.c_double), float(damping), _ptr(dx, C.c_double)))
        return dx

    def ik_solve(self, x0, fixed=None, tgt_pos=None, tgt_rot=None, w_lin=None, w_ang=None, lo=None, hi=None, damping=None,
                 max_iters=None, tol: float = 0.0, max_step: float = 0.0):
        """-> (x (B, n_in) float64, iters (B) int32, err (B) float64) (dexr_link_ik_solve); at least one of tgt_pos
        (B, n_link, 3), tgt_rot (B, n_link, 3, 3) is required, w_lin, w_ang (B, n_link) or None weigh them, lo, hi (n_in) are
        given together or not at all, damping > 0 and max_iters in 1..256 are required."""
        if damping is None:
            raise ValueError("damping is required")
        if max_iters is None:
            raise ValueError("max_iters is required")
        x0, fixed, B = self._host_inputs(x0, fixed)
        tgt_pos = self._host_link_rows(tgt_pos, B, "tgt_pos")
        if tgt_rot is not None:
            tgt_rot = np.ascontiguousarray(tgt_rot, dtype=np.float64)
            if tgt_rot.shape != (B, self.n_link, 3, 3):
                raise ValueError(f"tgt_rot must have shape ({B}, {self.n_link}, 3, 3), got {tgt_rot.shape}")
        w_lin, w_ang = self._host_link_weights(w_lin, B, "w_lin"), self._host_link_weights(w_ang, B, "w_ang")
        if (lo is None) != (hi is None):
            raise ValueError("lo and hi must both be given or both be None")
        if lo is not None:
            lo, hi = (np.ascontiguousarray(a, dtype=np.float64) for a in (lo, hi))
            if lo.shape != (self.n_in,) or hi.shape != (self.n_in,):
                raise ValueError(f"lo and hi must have shape ({self.n_in},), got {lo.shape} and {hi.shape}")
        x = np.zeros((B, self.n_in), dtype=np.float64)
        iters = np.zeros(B, dtype=np.int32)
        err = np.zeros(B, dtype=np.float64)
        check(load().dexr_link_ik_solve(self._h, B, _ptr(x0, C.c_double), _ptr(fixed, C.c_double), _ptr(tgt_pos, C.c_double),
                                        _ptr(tgt_rot, C.c_double), _ptr(w_lin, C.c_double), _ptr(w_ang, C.c_double),
                                        _ptr(lo, C.c_double), _ptr(hi, C.c_double), float(damping), float(max_step), float(tol),
                                        int(max_iters), _ptr(x, C.c_double), _ptr(iters, C.c_int32), _ptr(err, C.c_double)))
        return x, iters, err

    def wrenches(self, x, fixed=None, force=None, torque=None, frame: int = 0):
        """-> tau (B, n_in) float64 (dexr_link_wrenches); at least one of force, torque (B, n_link, 3) is required."""
        x, fixed, B = self._host_inputs(x, fixed)
        force, torque = self._host_link_rows(force, B, "force"), self._host_link_rows(torque, B, "torque")
        tau = np.zeros((B, self.n_in), dtype=np.float64)
        check(load().dexr_link_wrenches(self._h, B, _ptr(x, C.c_double), _ptr(fixed, C.c_double), int(frame),
                                        _ptr(force, C.c_double), _ptr(torque, C.c_double), _ptr(tau, C.c_double)))
        return tau

    def velocities_vjp(self, x, xdot, fixed=None, grad_lin=None, grad_ang=None, frame: int = 0, want_x: bool = True,
                       want_xdot: bool = True):
        """-> (grad_x, grad_xdot) (B, n_in) float64, None where not wanted (dexr_link_velocities_vjp); at least one of
        grad_lin, grad_ang (B, n_link, 3) is required."""
        x, fixed, B = self._host_inputs(x, fixed)
        xdot = np.ascontiguousarray(np.atleast_2d(np.asarray(xdot, dtype=np.float64)))
        if xdot.shape != x.shape:
            raise ValueError(f"xdot must have the shape of x {x.shape}, got {xdot.shape}")
        grad_lin, grad_ang = self._host_link_rows(grad_lin, B, "grad_lin"), self._host_link_rows(grad_ang, B, "grad_ang")
        gx = np.zeros((B, self.n_in), dtype=np.float64) if want_x else None
        gxd = np.zeros((B, self.n_in), dtype=np.float64) if want_xdot else None
        check(load().dexr_link_velocities_vjp(self._h, B, _ptr(x, C.c_double), _ptr(fixed, C.c_double), _ptr(xdot, C.c_double),
                                              int(frame), _ptr(grad_lin, C.c_double), _ptr(grad_ang, C.c_double),
                                              _ptr(gx, C.c_double), _ptr(gxd, C.c_double)))
        return gx, gxd


class SphereModel:
    """Owns one dexr_sphere_model (include/dexr_spheres.h): the pose table of a list of links with spheres on them and a list
    of sphere pairs, resident in HBM.  sphere_link (S) rows of the link list, center (S, 3) in the link's frame, radius (S),
    pair (P, 2) sphere indices."""

    def __init__(self, pose_blob: bytes, sphere_link, center, radius, pair):
        lib = load()
        self._h = C.c_void_p()
        link = np.ascontiguousarray(sphere_link, dtype=np.int32).reshape(-1)
        cen = np.ascontiguousarray(center, dtype=np.float64).reshape(-1, 3)
        rad = np.ascontiguousarray(radius, dtype=np.float64).reshape(-1)
        pr = np.ascontiguousarray(pair, dtype=np.int32).reshape(-1, 2)
        if not (len(link) == len(cen) == len(rad)):
            raise ValueError(f"sphere_link, center and radius must have one row per sphere, got {len(link)}, {len(cen)}, {len(rad)}")
        buf = C.create_string_buffer(pose_blob, len(pose_blob))
        check(lib.dexr_sphere_model_create(buf, len(pose_blob), len(link), _ptr(link, C.c_int32), _ptr(cen, C.c_double),
                                           _ptr(rad, C.c_double), len(pr), _ptr(pr, C.c_int32), C.byref(self._h)))
        v = [C.c_int32() for _ in range(4)]
        check(lib.dexr_sphere_model_info(self._h, *[C.byref(a) for a in v]))
        self.n_in, self.n_fixed, self.n_sphere, self.n_pair = (int(a.value) for a in v)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib is not None:
            _lib.dexr_sphere_model_destroy(h)
            self._h = None

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    # device-pointer entry points: float32, C-contiguous, enqueued on `stream` ------------------------
    def distances_dev(self, B: int, x_ptr: int, fixed_ptr: int, dist_ptr: int, center_ptr: int = 0, stream: int = 0):
        """x (B, n_in), fixed (B, n_fixed) or 0 -> dist (B, n_pair), center (B, n_sphere, 3) or 0 (dexr_sphere_distances_dev)."""
        check(load().dexr_sphere_distances_dev(self._h, B, x_ptr or None, fixed_ptr or None, dist_ptr or None, center_ptr or None,
                                               stream or None))

    def distances_vjp_dev(self, B: int, x_ptr: int, fixed_ptr: int, grad_dist_ptr: int, grad_x_ptr: int, stream: int = 0):
        """grad_dist (B, n_pair) -> grad_x (B, n_in), every entry written (dexr_sphere_distances_vjp_dev)."""
        check(load().dexr_sphere_distances_vjp_dev(self._h, B, x_ptr or None, fixed_ptr or None, grad_dist_ptr or None,
                                                   grad_x_ptr or None, stream or None))

    def penalty_dev(self, B: int, x_ptr: int, fixed_ptr: int, margin: float, pair_weight_ptr: int, energy_ptr: int, grad_x_ptr: int,
                    stream: int = 0):
        """margin >= 0, pair_weight (n_pair) or 0 (weights of 1) -> energy (B) and / or grad_x (B, n_in), either may be 0, from
        one launch (dexr_sphere_penalty_dev)."""
        check(load().dexr_sphere_penalty_dev(self._h, B, x_ptr or None, fixed_ptr or None, float(margin), pair_weight_ptr or None,
                                             energy_ptr or None, grad_x_ptr or None, stream or None))

    # host-pointer entry points: float64 in, float64 arithmetic, float64 out ----------------------------
    _host_inputs = PoseModel._host_inputs

    def distances(self, x, fixed=None, centers: bool = False):
        """-> dist (B, n_pair), centers (B, n_sphere, 3) or None; float64 (dexr_sphere_distances)."""
        x, fixed, B = self._host_inputs(x, fixed)
        dist = np.zeros((B, self.n_pair), dtype=np.float64)
        cen = np.zeros((B, self.n_sphere, 3), dtype=np.float64) if centers else None
        check(load().dexr_sphere_distances(self._h, B, _ptr(x, C.c_double), _ptr(fixed, C.c_double), _ptr(dist, C.c_double),
                                           _ptr(cen, C.c_double)))
        return dist, cen

    def distances_vjp(self, x, grad_dist, fixed=None):
        """-> grad_x (B, n_in) float64 (dexr_sphere_distances_vjp)."""
        x, fixed, B = self._host_inputs(x, fixed)
        grad_dist = np.ascontiguousarray(grad_dist, dtype=np.float64)
        if grad_dist.shape != (B, self.n_pair):
            raise ValueError(f"grad_dist must have shape ({B}, {self.n_pair}), got {grad_dist.shape}")
        gx = np.zeros((B, self.n_in), dtype=np.float64)
        check(load().dexr_sphere_distances_vjp(self._h, B, _ptr(x, C.c_double), _ptr(fixed, C.c_double), _ptr(grad_dist, C.c_double),
                                               _ptr(gx, C.c_double)))
        return gx

    def penalty(self, x, margin, pair_weight=None, fixed=None, want_energy: bool = True, want_grad: bool = True):
        """-> (energy (B), grad_x (B, n_in)) float64, None where not wanted (dexr_sphere_penalty)."""
        x, fixed, B = self._host_inputs(x, fixed)
        if pair_weight is not None:
            pair_weight = np.ascontiguousarray(pair_weight, dtype=np.float64)
            if pair_weight.shape != (self.n_pair,):
                raise ValueError(f"pair_weight must have shape ({self.n_pair},), got {pair_weight.shape}")
        e = np.zeros(B, dtype=np.float64) if want_energy else None
        gx = np.zeros((B, self.n_in), dtype=np.float64) if want_grad else None
        check(load().dexr_sphere_penalty(self._h, B, _ptr(x, C.c_double), _ptr(fixed, C.c_double), float(margin),
                                         _ptr(pair_weight, C.c_double), _ptr(e, C.c_double), _ptr(gx, C.c_double)))
        return e, gx

    # the collision-aware posture solve (include/dexr_resolve.h) ------------------------------------------
    def resolve_dev(self, B: int, x0_ptr: int, fixed_ptr: int, margin: float, damping: float, max_iters: int, x_ptr: int,
                    iters_ptr: int = 0, energy_ptr: int = 0, status_ptr: int = 0, x_ref_ptr: int = 0, posture_weight_ptr: int = 0,
                    n_target: int = 0, target_pos_ptr: int = 0, target_rot_ptr: int = 0, pos_weight_ptr: int = 0, rot_weight_ptr: int = 0,
                    collision_weight: float = 1.0, pair_weight_ptr: int = 0, lo_ptr: int = 0, hi_ptr: int = 0, tol: float = 0.0,
                    max_step: float = 0.0, stream: int = 0):
        """x0 (B, n_in), x_ref (B, n_in) or 0 (x0), posture_weight (n_in) or 0, the first n_target links of the table as targets:
        target_pos (B, n_target, 3) and / or target_rot (B, n_target, 3, 3), pos_weight, rot_weight (B, n_target) or 0,
        pair_weight (n_pair) or 0, lo, hi (n_in) or both 0 -> x (B, n_in), iters (B) int32, energy (B, 3), status (B) int32, each
        of the last three or 0: up to max_iters trial steps inside one launch; x may alias x0 (dexr_sphere_resolve_dev)."""
        check(load().dexr_sphere_resolve_dev(self._h, B, x0_ptr or None, fixed_ptr or None, x_ref_ptr or None, posture_weight_ptr or None,
                                             int(n_target), target_pos_ptr or None, target_rot_ptr or None, pos_weight_ptr or None,
                                             rot_weight_ptr or None, float(margin), float(collision_weight), pair_weight_ptr or None,
                                             lo_ptr or None, hi_ptr or None, float(damping), float(max_step), float(tol), int(max_iters),
                                             x_ptr or None, iters_ptr or None, energy_ptr or None, status_ptr or None, stream or None))

    def resolve(self, x0, margin=None, damping=None, max_iters=None, fixed=None, x_ref=None, posture_weight=None, target_pos=None,
                target_rot=None, pos_weight=None, rot_weight=None, collision_weight: float = 1.0, pair_weight=None, lo=None, hi=None,
                tol: float = 0.0, max_step: float = 0.0, n_target=None):
        """-> (x (B, n_in) float64, iters (B) int32, energy (B, 3) float64, status (B) int32) (dexr_sphere_resolve).  The
        targets are the first n_target links of the table; n_target is read from the shape of target_pos / target_rot
        ((B, n_target, 3) / (B, n_target, 3, 3)) unless given.  margin, damping > 0 and max_iters in 1..256 are required."""
        (x0, fixed, x_ref, posture_weight, target_pos, target_rot, pos_weight, rot_weight, pair_weight, lo, hi), n_target, B, out = \
            self._resolve_host(x0, margin, damping, max_iters, fixed, x_ref, posture_weight, target_pos, target_rot, pos_weight, rot_weight,
                               pair_weight, lo, hi, n_target, 3)
        x, iters, energy, status = out
        d = lambda a: _ptr(a, C.c_double)  # noqa: E731
        check(load().dexr_sphere_resolve(self._h, B, d(x0), d(fixed), d(x_ref), d(posture_weight), n_target, d(target_pos), d(target_rot),
                                         d(pos_weight), d(rot_weight), float(margin), float(collision_weight), d(pair_weight), d(lo), d(hi),
                                         float(damping), float(max_step), float(tol), int(max_iters), d(x), _ptr(iters, C.c_int32),
                                         d(energy), _ptr(status, C.c_int32)))
        return out

    def _resolve_host(self, x0, margin, damping, max_iters, fixed, x_ref, posture_weight, target_pos, target_rot, pos_weight, rot_weight,
                      pair_weight, lo, hi, n_target, energy_cols, pose=None, extra=()):
        """What the three host resolve methods share, in the order their rules fire: the required scalars, x0 and fixed, every array
        as contiguous float64 (extra: (name, array, a callable that gives its shape, asked when the table is built) of the caller's own, last in the shape
        table), the obstacle pose where
        pose = (obstacle_pos, obstacle_rot) is given, n_target from the shape of the targets unless given, the shape table, the
        lo / hi rule and the four outputs.  -> ((x0, fixed, the nine arrays in argument order[, pos, rot], the extra arrays),
        n_target, B, (x, iters, energy (B, energy_cols), status))."""
        for name, v in (("margin", margin), ("damping", damping), ("max_iters", max_iters)):
            if v is None:
                raise ValueError(f"{name} is required")
        x0, fixed, B = self._host_inputs(x0, fixed)
        f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
        x_ref, posture_weight, target_pos, target_rot, pos_weight, rot_weight, pair_weight, lo, hi = (
            f64(a) for a in (x_ref, posture_weight, target_pos, target_rot, pos_weight, rot_weight, pair_weight, lo, hi))
        extra = [(name, f64(a), want) for name, a, want in extra]
        posed = () if pose is None else self._host_pose(B, *pose)
        if n_target is None:
            n_target = 0 if target_pos is None and target_rot is None else (target_pos if target_pos is not None else target_rot).shape[1]
        n_target = int(n_target)
        shapes = [("x_ref", x_ref, (B, self.n_in)), ("posture_weight", posture_weight, (self.n_in,)), ("target_pos", target_pos, (B, n_target, 3)),
                  ("target_rot", target_rot, (B, n_target, 3, 3)), ("pos_weight", pos_weight, (B, n_target)),
                  ("rot_weight", rot_weight, (B, n_target)), ("pair_weight", pair_weight, (self.n_pair,)), ("lo", lo, (self.n_in,)),
                  ("hi", hi, (self.n_in,))] + [(name, a, want()) for name, a, want in extra]
        for name, a, want in shapes:
            if a is not None and a.shape != want:
                raise ValueError(f"{name} must have shape {want}, got {a.shape}")
        if (lo is None) != (hi is None):
            raise ValueError("lo and hi must both be given or both be None")
        out = (np.zeros((B, self.n_in), dtype=np.float64), np.zeros(B, dtype=np.int32), np.zeros((B, energy_cols), dtype=np.float64),
               np.zeros(B, dtype=np.int32))
        arrays = (x0, fixed, x_ref, posture_weight, target_pos, target_rot, pos_weight, rot_weight, pair_weight, lo, hi, *posed,
                  *(a for _, a, _ in extra))
        return arrays, n_target, B, out

    # the posture solve with the obstacle term (include/dexr_resolve_obstacles.h) --------------------------------
    def resolve_obstacles_dev(self, obstacles: "ObstacleSet", B: int, x0_ptr: int, fixed_ptr: int, margin: float, damping: float,
                              max_iters: int, x_ptr: int, iters_ptr: int = 0, energy_ptr: int = 0, status_ptr: int = 0, x_ref_ptr: int = 0,
                              posture_weight_ptr: int = 0, n_target: int = 0, target_pos_ptr: int = 0, target_rot_ptr: int = 0,
                              pos_weight_ptr: int = 0, rot_weight_ptr: int = 0, collision_weight: float = 1.0, pair_weight_ptr: int = 0,
                              lo_ptr: int = 0, hi_ptr: int = 0, tol: float = 0.0, max_step: float = 0.0, obstacle_pos_ptr: int = 0,
                              obstacle_rot_ptr: int = 0, obstacle_margin=None, obstacle_weight: float = 1.0, prim_weight_ptr: int = 0,
                              stream: int = 0):
        """the arguments of resolve_dev, and obstacle_pos (B, 3) or 0, obstacle_rot (B, 3, 3) or 0, obstacle_margin (None: margin),
        obstacle_weight, prim_weight (n_prim) or 0 -> x (B, n_in), iters (B) int32, energy (B, 4), status (B) int32, each of the last
        three or 0 (dexr_sphere_resolve_obstacles_dev)."""
        om = margin if obstacle_margin is None else obstacle_margin
        check(load().dexr_sphere_resolve_obstacles_dev(
            self._h, B, x0_ptr or None, fixed_ptr or None, x_ref_ptr or None, posture_weight_ptr or None, int(n_target), target_pos_ptr or None,
            target_rot_ptr or None, pos_weight_ptr or None, rot_weight_ptr or None, float(margin), float(collision_weight), pair_weight_ptr or None,
            lo_ptr or None, hi_ptr or None, float(damping), float(max_step), float(tol), int(max_iters), obstacles.handle, obstacle_pos_ptr or None,
            obstacle_rot_ptr or None, float(om), float(obstacle_weight), prim_weight_ptr or None, x_ptr or None, iters_ptr or None,
            energy_ptr or None, status_ptr or None, stream or None))

    def resolve_obstacles(self, obstacles: "ObstacleSet", x0, margin=None, damping=None, max_iters=None, fixed=None, x_ref=None,
                          posture_weight=None, target_pos=None, target_rot=None, pos_weight=None, rot_weight=None,
                          collision_weight: float = 1.0, pair_weight=None, lo=None, hi=None, tol: float = 0.0, max_step: float = 0.0,
                          n_target=None, obstacle_pos=None, obstacle_rot=None, obstacle_margin=None, obstacle_weight: float = 1.0,
                          prim_weight=None):
        """-> (x (B, n_in) float64, iters (B) int32, energy (B, 4) float64, status (B) int32) (dexr_sphere_resolve_obstacles): the
        arguments of `resolve`, and the obstacle pose per frame or None, obstacle_margin (None: margin), obstacle_weight and
        prim_weight (n_prim) or None."""
        (x0, fixed, x_ref, posture_weight, target_pos, target_rot, pos_weight, rot_weight, pair_weight, lo, hi, pos, rot,
         prim_weight), n_target, B, out = self._resolve_host(
            x0, margin, damping, max_iters, fixed, x_ref, posture_weight, target_pos, target_rot, pos_weight, rot_weight, pair_weight, lo, hi,
            n_target, 4, pose=(obstacle_pos, obstacle_rot), extra=(("prim_weight", prim_weight, lambda: (obstacles.n_prim,)),))
        x, iters, energy, status = out
        d = lambda a: _ptr(a, C.c_double)  # noqa: E731
        om = margin if obstacle_margin is None else obstacle_margin
        check(load().dexr_sphere_resolve_obstacles(
            self._h, B, d(x0), d(fixed), d(x_ref), d(posture_weight), n_target, d(target_pos), d(target_rot), d(pos_weight), d(rot_weight),
            float(margin), float(collision_weight), d(pair_weight), d(lo), d(hi), float(damping), float(max_step), float(tol), int(max_iters),
            obstacles.handle, d(pos), d(rot), float(om), float(obstacle_weight), d(prim_weight), d(x), _ptr(iters, C.c_int32), d(energy),
            _ptr(status, C.c_int32)))
        return out

    # the model's spheres against an obstacle set (include/dexr_obstacles.h); the pair list plays no part --------------
    def obstacle_distances_dev(self, obstacles: "ObstacleSet", B: int, x_ptr: int, fixed_ptr: int, dist_ptr: int, nearest_ptr: int = 0,
                               obstacle_pos_ptr: int = 0, obstacle_rot_ptr: int = 0, stream: int = 0):
        """x (B, n_in), fixed (B, n_fixed) or 0, obstacle_pos (B, 3) or 0, obstacle_rot (B, 3, 3) or 0 -> dist (B, n_sphere) and /
        or nearest (B, n_sphere) int32, either may be 0 (dexr_obstacle_distances_dev)."""
        check(load().dexr_obstacle_distances_dev(self._h, obstacles.handle, B, x_ptr or None, fixed_ptr or None, obstacle_pos_ptr or None,
                                                 obstacle_rot_ptr or None, dist_ptr or None, nearest_ptr or None, stream or None))

    def obstacle_distances_vjp_dev(self, obstacles: "ObstacleSet", B: int, x_ptr: int, fixed_ptr: int, grad_dist_ptr: int, grad_x_ptr: int,
                                   obstacle_pos_ptr: int = 0, obstacle_rot_ptr: int = 0, stream: int = 0):
        """grad_dist (B, n_sphere) -> grad_x (B, n_in), every entry written (dexr_obstacle_distances_vjp_dev)."""
        check(load().dexr_obstacle_distances_vjp_dev(self._h, obstacles.handle, B, x_ptr or None, fixed_ptr or None, obstacle_pos_ptr or None,
                                                     obstacle_rot_ptr or None, grad_dist_ptr or None, grad_x_ptr or None, stream or None))

    def obstacle_penalty_dev(self, obstacles: "ObstacleSet", B: int, x_ptr: int, fixed_ptr: int, margin: float, prim_weight_ptr: int,
                             energy_ptr: int, grad_x_ptr: int, wrench_ptr: int = 0, obstacle_pos_ptr: int = 0, obstacle_rot_ptr: int = 0,
                             stream: int = 0):
        """margin >= 0, prim_weight (n_prim) or 0 (weights of 1) -> energy (B), grad_x (B, n_in), wrench (B, 6), each may be 0 but
        not all, from one launch (dexr_obstacle_penalty_dev)."""
        check(load().dexr_obstacle_penalty_dev(self._h, obstacles.handle, B, x_ptr or None, fixed_ptr or None, obstacle_pos_ptr or None,
                                               obstacle_rot_ptr or None, float(margin), prim_weight_ptr or None, energy_ptr or None,
                                               grad_x_ptr or None, wrench_ptr or None, stream or None))

    @staticmethod
    def _host_pose(B, obstacle_pos, obstacle_rot):
        out = []
        for name, a, shape in (("obstacle_pos", obstacle_pos, (B, 3)), ("obstacle_rot", obstacle_rot, (B, 3, 3))):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape != shape:
                    raise ValueError(f"{name} must have shape {shape}, got {a.shape}")
            out.append(a)
        return out

    def obstacle_distances(self, obstacles: "ObstacleSet", x, fixed=None, obstacle_pos=None, obstacle_rot=None, nearest: bool = True):
        """-> dist (B, n_sphere) float64, nearest (B, n_sphere) int32 or None (dexr_obstacle_distances)."""
        x, fixed, B = self._host_inputs(x, fixed)
        pos, rot = self._host_pose(B, obstacle_pos, obstacle_rot)
        dist = np.zeros((B, self.n_sphere), dtype=np.float64)
        near = np.zeros((B, self.n_sphere), dtype=np.int32) if nearest else None
        d = lambda a: _ptr(a, C.c_double)  # noqa: E731
        check(load().dexr_obstacle_distances(self._h, obstacles.handle, B, d(x), d(fixed), d(pos), d(rot), d(dist), _ptr(near, C.c_int32)))
        return dist, near

    def obstacle_distances_vjp(self, obstacles: "ObstacleSet", x, grad_dist, fixed=None, obstacle_pos=None, obstacle_rot=None):
        """-> grad_x (B, n_in) float64 (dexr_obstacle_distances_vjp)."""
        x, fixed, B = self._host_inputs(x, fixed)
        pos, rot = self._host_pose(B, obstacle_pos, obstacle_rot)
        grad_dist = np.ascontiguousarray(grad_dist, dtype=np.float64)
        if grad_dist.shape != (B, self.n_sphere):
            raise ValueError(f"grad_dist must have shape ({B}, {self.n_sphere}), got {grad_dist.shape}")
        gx = np.zeros((B, self.n_in), dtype=np.float64)
        d = lambda a: _ptr(a, C.c_double)  # noqa: E731
        check(load().dexr_obstacle_distances_vjp(self._h, obstacles.handle, B, d(x), d(fixed), d(pos), d(rot), d(grad_dist), d(gx)))
        return gx

    def obstacle_penalty(self, obstacles: "ObstacleSet", x, margin, prim_weight=None, fixed=None, obstacle_pos=None, obstacle_rot=None,
                         want_energy: bool = True, want_grad: bool = True, want_wrench: bool = True):
        """-> (energy (B), grad_x (B, n_in), wrench (B, 6)) float64, None where not wanted (dexr_obstacle_penalty)."""
        x, fixed, B = self._host_inputs(x, fixed)
        pos, rot = self._host_pose(B, obstacle_pos, obstacle_rot)
        if prim_weight is not None:
            prim_weight = np.ascontiguousarray(prim_weight, dtype=np.float64)
            if prim_weight.shape != (obstacles.n_prim,):
                raise ValueError(f"prim_weight must have shape ({obstacles.n_prim},), got {prim_weight.shape}")
        e = np.zeros(B, dtype=np.float64) if want_energy else None
        gx = np.zeros((B, self.n_in), dtype=np.float64) if want_grad else None
        wr = np.zeros((B, 6), dtype=np.float64) if want_wrench else None
        d = lambda a: _ptr(a, C.c_double)  # noqa: E731
        check(load().dexr_obstacle_penalty(self._h, obstacles.handle, B, d(x), d(fixed), d(pos), d(rot), float(margin), d(prim_weight), d(e),
                                           d(gx), d(wr)))
        return e, gx, wr

    # the model's spheres against another posed model's (include/dexr_cross.h); self is robot A, neither pair list plays a part ----
    def cross_distances_dev(self, other: "SphereModel", B: int, x_a_ptr: int, fixed_a_ptr: int, x_b_ptr: int, fixed_b_ptr: int,
                            dist_a_ptr: int = 0, nearest_a_ptr: int = 0, dist_b_ptr: int = 0, nearest_b_ptr: int = 0, pos_a_ptr: int = 0,
                            rot_a_ptr: int = 0, pos_b_ptr: int = 0, rot_b_ptr: int = 0, stream: int = 0):
        """x_a (B, n_in_a), x_b (B, n_in_b), fixed_* or 0, pos_* (B, 3) or 0, rot_* (B, 3, 3) or 0 -> dist_a (B, S_a), nearest_a
        (B, S_a) int32, dist_b (B, S_b), nearest_b (B, S_b) int32, each may be 0, not all (dexr_cross_distances_dev)."""
        check(load().dexr_cross_distances_dev(self._h, other.handle, B, x_a_ptr or None, fixed_a_ptr or None, x_b_ptr or None,
                                              fixed_b_ptr or None, pos_a_ptr or None, rot_a_ptr or None, pos_b_ptr or None, rot_b_ptr or None,
                                              dist_a_ptr or None, nearest_a_ptr or None, dist_b_ptr or None, nearest_b_ptr or None,
                                              stream or None))

    def cross_distances_vjp_dev(self, other: "SphereModel", B: int, x_a_ptr: int, fixed_a_ptr: int, x_b_ptr: int, fixed_b_ptr: int,
                                grad_dist_a_ptr: int, grad_dist_b_ptr: int, grad_xa_ptr: int, grad_xb_ptr: int, wrench_a_ptr: int = 0,
                                wrench_b_ptr: int = 0, pos_a_ptr: int = 0, rot_a_ptr: int = 0, pos_b_ptr: int = 0, rot_b_ptr: int = 0,
                                stream: int = 0):
        """grad_dist_a (B, S_a) or 0, grad_dist_b (B, S_b) or 0 -> grad_xa (B, n_in_a), grad_xb (B, n_in_b), wrench_a, wrench_b
        (B, 6) or 0, every entry written (dexr_cross_distances_vjp_dev)."""
        check(load().dexr_cross_distances_vjp_dev(self._h, other.handle, B, x_a_ptr or None, fixed_a_ptr or None, x_b_ptr or None,
                                                  fixed_b_ptr or None, pos_a_ptr or None, rot_a_ptr or None, pos_b_ptr or None,
                                                  rot_b_ptr or None, grad_dist_a_ptr or None, grad_dist_b_ptr or None, grad_xa_ptr or None,
                                                  grad_xb_ptr or None, wrench_a_ptr or None, wrench_b_ptr or None, stream or None))

    def cross_penalty_dev(self, other: "SphereModel", B: int, x_a_ptr: int, fixed_a_ptr: int, x_b_ptr: int, fixed_b_ptr: int, margin: float,
                          pair_weight_ptr: int, energy_ptr: int, grad_xa_ptr: int, grad_xb_ptr: int, wrench_a_ptr: int = 0,
                          wrench_b_ptr: int = 0, pos_a_ptr: int = 0, rot_a_ptr: int = 0, pos_b_ptr: int = 0, rot_b_ptr: int = 0,
                          stream: int = 0):
        """margin >= 0, pair_weight (S_a, S_b) or 0 -> energy (B), grad_xa (B, n_in_a), grad_xb (B, n_in_b), wrench_a, wrench_b
        (B, 6), each may be 0, not all, from one launch (dexr_cross_penalty_dev)."""
        check(load().dexr_cross_penalty_dev(self._h, other.handle, B, x_a_ptr or None, fixed_a_ptr or None, x_b_ptr or None,
                                            fixed_b_ptr or None, pos_a_ptr or None, rot_a_ptr or None, pos_b_ptr or None, rot_b_ptr or None,
                                            float(margin), pair_weight_ptr or None, energy_ptr or None, grad_xa_ptr or None,
                                            grad_xb_ptr or None, wrench_a_ptr or None, wrench_b_ptr or None, stream or None))

    def _cross_host(self, other, x_a, x_b, fixed_a, fixed_b, pos_a, rot_a, pos_b, rot_b):
        x_a, fixed_a, B = self._host_inputs(x_a, fixed_a)
        x_b, fixed_b, Bb = other._host_inputs(x_b, fixed_b)
        if Bb != B:
            raise ValueError(f"x_a has {B} frames, x_b {Bb}: both robots need one row per frame")
        poses = []
        for name, a, shape in (("pos_a", pos_a, (B, 3)), ("rot_a", rot_a, (B, 3, 3)), ("pos_b", pos_b, (B, 3)), ("rot_b", rot_b, (B, 3, 3))):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape != shape:
                    raise ValueError(f"{name} must have shape {shape}, got {a.shape}")
            poses.append(a)
        return B, [_ptr(a, C.c_double) for a in (x_a, fixed_a, x_b, fixed_b, *poses)], (x_a, fixed_a, x_b, fixed_b, poses)

    def cross_distances(self, other: "SphereModel", x_a, x_b, fixed_a=None, fixed_b=None, pos_a=None, rot_a=None, pos_b=None, rot_b=None,
                        nearest: bool = True):
        """-> dist_a (B, S_a), nearest_a (B, S_a) int32 or None, dist_b (B, S_b), nearest_b or None; float64 (dexr_cross_distances)."""
        B, ptrs, _keep = self._cross_host(other, x_a, x_b, fixed_a, fixed_b, pos_a, rot_a, pos_b, rot_b)
        da, db = np.zeros((B, self.n_sphere), dtype=np.float64), np.zeros((B, other.n_sphere), dtype=np.float64)
        na = np.zeros((B, self.n_sphere), dtype=np.int32) if nearest else None
        nb = np.zeros((B, other.n_sphere), dtype=np.int32) if nearest else None
        check(load().dexr_cross_distances(self._h, other.handle, B, *ptrs, _ptr(da, C.c_double), _ptr(na, C.c_int32), _ptr(db, C.c_double),
                                          _ptr(nb, C.c_int32)))
        return da, na, db, nb

    def cross_distances_vjp(self, other: "SphereModel", x_a, x_b, grad_dist_a=None, grad_dist_b=None, fixed_a=None, fixed_b=None,
                            pos_a=None, rot_a=None, pos_b=None, rot_b=None, want_wrench: bool = True):
        """-> (grad_xa (B, n_in_a), grad_xb (B, n_in_b), wrench_a, wrench_b (B, 6) or None) float64 (dexr_cross_distances_vjp)."""
        B, ptrs, _keep = self._cross_host(other, x_a, x_b, fixed_a, fixed_b, pos_a, rot_a, pos_b, rot_b)
        gd = []
        for name, g, n in (("grad_dist_a", grad_dist_a, self.n_sphere), ("grad_dist_b", grad_dist_b, other.n_sphere)):
            if g is not None:
                g = np.ascontiguousarray(g, dtype=np.float64)
                if g.shape != (B, n):
                    raise ValueError(f"{name} must have shape ({B}, {n}), got {g.shape}")
            gd.append(g)
        gxa, gxb = np.zeros((B, self.n_in), dtype=np.float64), np.zeros((B, other.n_in), dtype=np.float64)
        wa = np.zeros((B, 6), dtype=np.float64) if want_wrench else None
        wb = np.zeros((B, 6), dtype=np.float64) if want_wrench else None
        d = lambda a: _ptr(a, C.c_double)  # noqa: E731
        check(load().dexr_cross_distances_vjp(self._h, other.handle, B, *ptrs, d(gd[0]), d(gd[1]), d(gxa), d(gxb), d(wa), d(wb)))
        return gxa, gxb, wa, wb

    def cross_penalty(self, other: "SphereModel", x_a, x_b, margin, pair_weight=None, fixed_a=None, fixed_b=None, pos_a=None, rot_a=None,
                      pos_b=None, rot_b=None, want_energy: bool = True, want_grad_a: bool = True, want_grad_b: bool = True,
                      want_wrench_a: bool = True, want_wrench_b: bool = True):
        """-> (energy (B), grad_xa, grad_xb, wrench_a (B, 6), wrench_b (B, 6)) float64, None where not wanted (dexr_cross_penalty)."""
        B, ptrs, _keep = self._cross_host(other, x_a, x_b, fixed_a, fixed_b, pos_a, rot_a, pos_b, rot_b)
        if pair_weight is not None:
            pair_weight = np.ascontiguousarray(pair_weight, dtype=np.float64)
            if pair_weight.shape != (self.n_sphere, other.n_sphere):
                raise ValueError(f"pair_weight must have shape ({self.n_sphere}, {other.n_sphere}), got {pair_weight.shape}")
        e = np.zeros(B, dtype=np.float64) if want_energy else None
        gxa = np.zeros((B, self.n_in), dtype=np.float64) if want_grad_a else None
        gxb = np.zeros((B, other.n_in), dtype=np.float64) if want_grad_b else None
        wa = np.zeros((B, 6), dtype=np.float64) if want_wrench_a else None
        wb = np.zeros((B, 6), dtype=np.float64) if want_wrench_b else None
        d = lambda a: _ptr(a, C.c_double)  # noqa: E731
        check(load().dexr_cross_penalty(self._h, other.handle, B, *ptrs, float(margin), d(pair_weight), d(e), d(gxa), d(gxb), d(wa), d(wb)))
        return e, gxa, gxb, wa, wb

    # the model's spheres against a sampled signed-distance field (include/dexr_sdf_grid.h); the pair list plays no part ----
    def grid_distances_dev(self, grid: "SdfGrid", B: int, x_ptr: int, fixed_ptr: int, dist_ptr: int, obstacle_pos_ptr: int = 0,
                           obstacle_rot_ptr: int = 0, stream: int = 0):
        """x (B, n_in), fixed (B, n_fixed) or 0, obstacle_pos (B, 3) or 0, obstacle_rot (B, 3, 3) or 0 -> dist (B, n_sphere)
        (dexr_grid_distances_dev)."""
        check(load().dexr_grid_distances_dev(self._h, grid.handle, B, x_ptr or None, fixed_ptr or None, obstacle_pos_ptr or None,
                                             obstacle_rot_ptr or None, dist_ptr or None, stream or None))

    def grid_distances_vjp_dev(self, grid: "SdfGrid", B: int, x_ptr: int, fixed_ptr: int, grad_dist_ptr: int, grad_x_ptr: int,
                               obstacle_pos_ptr: int = 0, obstacle_rot_ptr: int = 0, stream: int = 0):
        """grad_dist (B, n_sphere) -> grad_x (B, n_in), every entry written (dexr_grid_distances_vjp_dev)."""
        check(load().dexr_grid_distances_vjp_dev(self._h, grid.handle, B, x_ptr or None, fixed_ptr or None, obstacle_pos_ptr or None,
                                                 obstacle_rot_ptr or None, grad_dist_ptr or None, grad_x_ptr or None, stream or None))

    def grid_penalty_dev(self, grid: "SdfGrid", B: int, x_ptr: int, fixed_ptr: int, margin: float, energy_ptr: int, grad_x_ptr: int,
                         wrench_ptr: int = 0, obstacle_pos_ptr: int = 0, obstacle_rot_ptr: int = 0, stream: int = 0):
        """margin >= 0 -> energy (B), grad_x (B, n_in), wrench (B, 6), each may be 0 but not all, from one launch
        (dexr_grid_penalty_dev)."""
        check(load().dexr_grid_penalty_dev(self._h, grid.handle, B, x_ptr or None, fixed_ptr or None, obstacle_pos_ptr or None,
                                           obstacle_rot_ptr or None, float(margin), energy_ptr or None, grad_x_ptr or None,
                                           wrench_ptr or None, stream or None))

    def grid_distances(self, grid: "SdfGrid", x, fixed=None, obstacle_pos=None, obstacle_rot=None):
        """-> dist (B, n_sphere) float64 (dexr_grid_distances)."""
        x, fixed, B = self._host_inputs(x, fixed)
        pos, rot = self._host_pose(B, obstacle_pos, obstacle_rot)
        dist = np.zeros((B, self.n_sphere), dtype=np.float64)
        d = lambda a: _ptr(a, C.c_double)  # noqa: E731
        check(load().dexr_grid_distances(self._h, grid.handle, B, d(x), d(fixed), d(pos), d(rot), d(dist)))
        return dist

    def grid_distances_vjp(self, grid: "SdfGrid", x, grad_dist, fixed=None, obstacle_pos=None, obstacle_rot=None):
        """-> grad_x (B, n_in) float64 (dexr_grid_distances_vjp)."""
        x, fixed, B = self._host_inputs(x, fixed)
        pos, rot = self._host_pose(B, obstacle_pos, obstacle_rot)
        grad_dist = np.ascontiguousarray(grad_dist, dtype=np.float64)
        if grad_dist.shape != (B, self.n_sphere):
            raise ValueError(f"grad_dist must have shape ({B}, {self.n_sphere}), got {grad_dist.shape}")
        gx = np.zeros((B, self.n_in), dtype=np.float64)
        d = lambda a: _ptr(a, C.c_double)  # noqa: E731
        check(load().dexr_grid_distances_vjp(self._h, grid.handle, B, d(x), d(fixed), d(pos), d(rot), d(grad_dist), d(gx)))
        return gx

    def grid_penalty(self, grid: "SdfGrid", x, margin, fixed=None, obstacle_pos=None, obstacle_rot=None, want_energy: bool = True,
                     want_grad: bool = True, want_wrench: bool = True):
        """-> (energy (B), grad_x (B, n_in), wrench (B, 6)) float64, None where not wanted (dexr_grid_penalty)."""
        x, fixed, B = self._host_inputs(x, fixed)
        pos, rot = self._host_pose(B, obstacle_pos, obstacle_rot)
        e = np.zeros(B, dtype=np.float64) if want_energy else None
        gx = np.zeros((B, self.n_in), dtype=np.float64) if want_grad else None
        wr = np.zeros((B, 6), dtype=np.float64) if want_wrench else None
        d = lambda a: _ptr(a, C.c_double)  # noqa: E731
        check(load().dexr_grid_penalty(self._h, grid.handle, B, d(x), d(fixed), d(pos), d(rot), float(margin), d(e), d(gx), d(wr)))
        return e, gx, wr

    # the posture solve with the grid term (include/dexr_resolve_grid.h) -----------------------------------------
    def resolve_grid_dev(self, grid: "SdfGrid", B: int, x0_ptr: int, fixed_ptr: int, margin: float, damping: float, max_iters: int,
                         x_ptr: int, iters_ptr: int = 0, energy_ptr: int = 0, status_ptr: int = 0, x_ref_ptr: int = 0,
                         posture_weight_ptr: int = 0, n_target: int = 0, target_pos_ptr: int = 0, target_rot_ptr: int = 0,
                         pos_weight_ptr: int = 0, rot_weight_ptr: int = 0, collision_weight: float = 1.0, pair_weight_ptr: int = 0,
                         lo_ptr: int = 0, hi_ptr: int = 0, tol: float = 0.0, max_step: float = 0.0, obstacle_pos_ptr: int = 0,
                         obstacle_rot_ptr: int = 0, obstacle_margin=None, obstacle_weight: float = 1.0, stream: int = 0):
        """the arguments of resolve_dev, and obstacle_pos (B, 3) or 0, obstacle_rot (B, 3, 3) or 0, obstacle_margin (None: margin),
        obstacle_weight -> x (B, n_in), iters (B) int32, energy (B, 4), status (B) int32, each of the last three or 0
        (dexr_sphere_resolve_grid_dev)."""
        om = margin if obstacle_margin is None else obstacle_margin
        check(load().dexr_sphere_resolve_grid_dev(
            self._h, B, x0_ptr or None, fixed_ptr or None, x_ref_ptr or None, posture_weight_ptr or None, int(n_target), target_pos_ptr or None,
            target_rot_ptr or None, pos_weight_ptr or None, rot_weight_ptr or None, float(margin), float(collision_weight), pair_weight_ptr or None,
            lo_ptr or None, hi_ptr or None, float(damping), float(max_step), float(tol), int(max_iters), grid.handle, obstacle_pos_ptr or None,
            obstacle_rot_ptr or None, float(om), float(obstacle_weight), x_ptr or None, iters_ptr or None, energy_ptr or None,
            status_ptr or None, stream or None))

    def resolve_grid(self, grid: "SdfGrid", x0, margin=None, damping=None, max_iters=None, fixed=None, x_ref=None, posture_weight=None,
                     target_pos=None, target_rot=None, pos_weight=None, rot_weight=None, collision_weight: float = 1.0, pair_weight=None,
                     lo=None, hi=None, tol: float = 0.0, max_step: float = 0.0, n_target=None, obstacle_pos=None, obstacle_rot=None,
                     obstacle_margin=None, obstacle_weight: float = 1.0):
        """-> (x (B, n_in) float64, iters (B) int32, energy (B, 4) float64, status (B) int32) (dexr_sphere_resolve_grid): the
        arguments of `resolve`, and the obstacle pose per frame or None, obstacle_margin (None: margin) and obstacle_weight."""
        (x0, fixed, x_ref, posture_weight, target_pos, target_rot, pos_weight, rot_weight, pair_weight, lo, hi, pos, rot), n_target, B, out = \
            self._resolve_host(x0, margin, damping, max_iters, fixed, x_ref, posture_weight, target_pos, target_rot, pos_weight, rot_weight,
                               pair_weight, lo, hi, n_target, 4, pose=(obstacle_pos, obstacle_rot))
        x, iters, energy, status = out
        d = lambda a: _ptr(a, C.c_double)  # noqa: E731
        om = margin if obstacle_margin is None else obstacle_margin
        check(load().dexr_sphere_resolve_grid(
            self._h, B, d(x0), d(fixed), d(x_ref), d(posture_weight), n_target, d(target_pos), d(target_rot), d(pos_weight), d(rot_weight),
            float(margin), float(collision_weight), d(pair_weight), d(lo), d(hi), float(damping), float(max_step), float(tol), int(max_iters),
            grid.handle, d(pos), d(rot), float(om), float(obstacle_weight), d(x), _ptr(iters, C.c_int32), d(energy), _ptr(status, C.c_int32)))
        return out

    # the posture solve against a scene of several bodies (include/dexr_resolve_scene.h) --------------------------
    @staticmethod
    def _scene_records(bodies, margin, address):
        """the dexr_scene_body array of `bodies`: (obstacle, pos, rot, margin or None (the solve's), weight, prim_weight) each, obstacle
        an ObstacleSet or an SdfGrid of this module; `address` turns pos, rot and prim_weight into addresses (0 / None: NULL)."""
        bodies = list(bodies)
        rec = (SceneBodyRecord * max(len(bodies), 1))()
        for r, (obstacle, pos, rot, bmargin, weight, prim_weight) in zip(rec, bodies):
            if isinstance(obstacle, ObstacleSet):
                r.set = obstacle.handle.value
            elif isinstance(obstacle, SdfGrid):
                r.grid = obstacle.handle.value
            elif obstacle is not None:
                raise ValueError(f"a body's obstacle must be an _lib.ObstacleSet or an _lib.SdfGrid, got {type(obstacle).__name__}")
            r.pos, r.rot, r.prim_weight = address(pos), address(rot), address(prim_weight)
            r.margin, r.weight = float(margin if bmargin is None else bmargin), float(weight)
        return len(bodies), (rec if bodies else None)

    def resolve_scene_dev(self, bodies, B: int, x0_ptr: int, fixed_ptr: int, margin: float, damping: float, max_iters: int, x_ptr: int,
                          iters_ptr: int = 0, energy_ptr: int = 0, status_ptr: int = 0, x_ref_ptr: int = 0, posture_weight_ptr: int = 0,
                          n_target: int = 0, target_pos_ptr: int = 0, target_rot_ptr: int = 0, pos_weight_ptr: int = 0,
                          rot_weight_ptr: int = 0, collision_weight: float = 1.0, pair_weight_ptr: int = 0, lo_ptr: int = 0, hi_ptr: int = 0,
                          tol: float = 0.0, max_step: float = 0.0, body_energy_ptr: int = 0, stream: int = 0):
        """the arguments of resolve_dev, and bodies: 1 .. SCENE_MAXBODY of (obstacle: ObstacleSet or SdfGrid, pos_ptr (B, 3) or 0,
        rot_ptr (B, 3, 3) or 0, margin or None (the solve's), weight, prim_weight_ptr (n_prim) or 0) -> x (B, n_in), iters (B) int32,
        energy (B, 4), status (B) int32, body_energy (B, n_body), each of the last four or 0 (dexr_sphere_resolve_scene_dev)."""
        n_body, rec = self._scene_records(bodies, margin, lambda a: a or None)
        check(load().dexr_sphere_resolve_scene_dev(
            self._h, B, x0_ptr or None, fixed_ptr or None, x_ref_ptr or None, posture_weight_ptr or None, int(n_target), target_pos_ptr or None,
            target_rot_ptr or None, pos_weight_ptr or None, rot_weight_ptr or None, float(margin), float(collision_weight), pair_weight_ptr or None,
            lo_ptr or None, hi_ptr or None, float(damping), float(max_step), float(tol), int(max_iters), n_body, rec, x_ptr or None,
            iters_ptr or None, energy_ptr or None, body_energy_ptr or None, status_ptr or None, stream or None))

    def resolve_scene(self, bodies, x0, margin=None, damping=None, max_iters=None, fixed=None, x_ref=None, posture_weight=None,
                      target_pos=None, target_rot=None, pos_weight=None, rot_weight=None, collision_weight: float = 1.0, pair_weight=None,
                      lo=None, hi=None, tol: float = 0.0, max_step: float = 0.0, n_target=None):
        """-> (x (B, n_in) float64, iters (B) int32, energy (B, 4) float64, status (B) int32, body_energy (B, n_body) float64)
        (dexr_sphere_resolve_scene): the arguments of `resolve`, and bodies: 1 .. SCENE_MAXBODY of (obstacle: ObstacleSet or SdfGrid,
        pos (B, 3) or None, rot (B, 3, 3) or None, margin or None (the solve's), weight, prim_weight (n_prim) or None)."""
        (x0, fixed, x_ref, posture_weight, target_pos, target_rot, pos_weight, rot_weight, pair_weight, lo, hi), n_target, B, out = \
            self._resolve_host(x0, margin, damping, max_iters, fixed, x_ref, posture_weight, target_pos, target_rot, pos_weight, rot_weight,
                               pair_weight, lo, hi, n_target, 4)
        x, iters, energy, status = out
        kept = []  # the float64 copies the records point into
        for b, (obstacle, pos, rot, bmargin, weight, prim_weight) in enumerate(bodies):
            pos, rot = self._host_pose(B, pos, rot)
            if prim_weight is not None:
                prim_weight = np.ascontiguousarray(prim_weight, dtype=np.float64)
                want = (getattr(obstacle, "n_prim", None),)
                if want[0] is not None and prim_weight.shape != want:
                    raise ValueError(f"prim_weight of body {b} must have shape {want}, got {prim_weight.shape}")
            kept.append((obstacle, pos, rot, bmargin, weight, prim_weight))
        n_body, rec = self._scene_records(kept, margin, lambda a: None if a is None else a.ctypes.data)
        body_energy = np.zeros((B, n_body), dtype=np.float64)
        d = lambda a: _ptr(a, C.c_double)  # noqa: E731
        check(load().dexr_sphere_resolve_scene(
            self._h, B, d(x0), d(fixed), d(x_ref), d(posture_weight), n_target, d(target_pos), d(target_rot), d(pos_weight), d(rot_weight),
            float(margin), float(collision_weight), d(pair_weight), d(lo), d(hi), float(damping), float(max_step), float(tol), int(max_iters),
            n_body, rec, d(x), _ptr(iters, C.c_int32), d(energy), d(body_energy), _ptr(status, C.c_int32)))
        return x, iters, energy, status, body_energy

    # the posture solve against a second posed robot (include/dexr_resolve_cross.h) ---------------------------------
    def resolve_cross_dev(self, other: "SphereModel", B: int, x0_ptr: int, fixed_ptr: int, x_b_ptr: int, fixed_b_ptr: int, margin: float,
                          damping: float, max_iters: int, x_ptr: int, iters_ptr: int = 0, energy_ptr: int = 0, status_ptr: int = 0,
                          x_ref_ptr: int = 0, posture_weight_ptr: int = 0, n_target: int = 0, target_pos_ptr: int = 0, target_rot_ptr: int = 0,
                          pos_weight_ptr: int = 0, rot_weight_ptr: int = 0, collision_weight: float = 1.0, pair_weight_ptr: int = 0,
                          lo_ptr: int = 0, hi_ptr: int = 0, tol: float = 0.0, max_step: float = 0.0, other_pos_ptr: int = 0,
                          other_rot_ptr: int = 0, cross_margin=None, cross_weight: float = 1.0, cross_pair_weight_ptr: int = 0,
                          stream: int = 0):
        """the arguments of resolve_dev, and the other robot: its model, x_b (B, n_in_b), fixed_b (B, n_fixed_b) or 0, other_pos (B, 3)
        or 0, other_rot (B, 3, 3) or 0 (its pose in this robot's root frame), cross_margin (None: margin), cross_weight (w_x),
        cross_pair_weight (S_a, S_b) or 0 -> x (B, n_in), iters (B) int32, energy (B, 4), status (B) int32, each of the last three or
        0 (dexr_sphere_resolve_cross_dev)."""
        xm = margin if cross_margin is None else cross_margin
        check(load().dexr_sphere_resolve_cross_dev(
            self._h, B, x0_ptr or None, fixed_ptr or None, x_ref_ptr or None, posture_weight_ptr or None, int(n_target), target_pos_ptr or None,
            target_rot_ptr or None, pos_weight_ptr or None, rot_weight_ptr or None, float(margin), float(collision_weight), pair_weight_ptr or None,
            lo_ptr or None, hi_ptr or None, float(damping), float(max_step), float(tol), int(max_iters), other.handle, x_b_ptr or None,
            fixed_b_ptr or None, other_pos_ptr or None, other_rot_ptr or None, float(xm), float(cross_weight), cross_pair_weight_ptr or None,
            x_ptr or None, iters_ptr or None, energy_ptr or None, status_ptr or None, stream or None))

    def resolve_cross(self, other: "SphereModel", x0, x_b, margin=None, damping=None, max_iters=None, fixed=None, fixed_b=None, x_ref=None,
                      posture_weight=None, target_pos=None, target_rot=None, pos_weight=None, rot_weight=None,
                      collision_weight: float = 1.0, pair_weight=None, lo=None, hi=None, tol: float = 0.0, max_step: float = 0.0,
                      n_target=None, other_pos=None, other_rot=None, cross_margin=None, cross_weight: float = 1.0, cross_pair_weight=None):
        """-> (x (B, n_in) float64, iters (B) int32, energy (B, 4) float64, status (B) int32) (dexr_sphere_resolve_cross): the
        arguments of `resolve`, and the other robot's model, x_b, fixed_b, its pose per frame or None, cross_margin (None: margin),
        cross_weight (w_x) and cross_pair_weight (S_a, S_b) or None."""
        (x0, fixed, x_ref, posture_weight, target_pos, target_rot, pos_weight, rot_weight, pair_weight, lo, hi, xw), n_target, B, out = \
            self._resolve_host(x0, margin, damping, max_iters, fixed, x_ref, posture_weight, target_pos, target_rot, pos_weight, rot_weight,
                               pair_weight, lo, hi, n_target, 4,
                               extra=[("cross_pair_weight", cross_pair_weight, lambda: (self.n_sphere, other.n_sphere))])
        x_b, fixed_b, Bb = other._host_inputs(x_b, fixed_b)
        if Bb != B:
            raise ValueError(f"x0 has {B} frames, x_b {Bb}: both robots need one row per frame")
        pos, rot = [], []
        for name, a, shape, to in (("other_pos", other_pos, (B, 3), pos), ("other_rot", other_rot, (B, 3, 3), rot)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape != shape:
                    raise ValueError(f"{name} must have shape {shape}, got {a.shape}")
            to.append(a)
        x, iters, energy, status = out
        d = lambda a: _ptr(a, C.c_double)  # noqa: E731
        xm = margin if cross_margin is None else cross_margin
        check(load().dexr_sphere_resolve_cross(
            self._h, B, d(x0), d(fixed), d(x_ref), d(posture_weight), n_target, d(target_pos), d(target_rot), d(pos_weight), d(rot_weight),
            float(margin), float(collision_weight), d(pair_weight), d(lo), d(hi), float(damping), float(max_step), float(tol), int(max_iters),
            other.handle, d(x_b), d(fixed_b), d(pos[0]), d(rot[0]), float(xm), float(cross_weight), d(xw), d(x), _ptr(iters, C.c_int32),
            d(energy), _ptr(status, C.c_int32)))
        return out


class ObstacleSet:
    """Owns one dexr_obstacle_set (include/dexr_obstacles.h): 1 .. OBSTACLE_MAX primitives of an obstacle frame, resident in HBM.
    kind (M) int32 of OBSTACLE_SPHERE / CAPSULE / BOX / HALFSPACE, param (M, OBSTACLE_PARAMS) float64.  Any SphereModel's
    obstacle_* methods take it."""

    def __init__(self, kind, param):
        lib = load()
        self._h = C.c_void_p()
        kind = np.ascontiguousarray(kind, dtype=np.int32).reshape(-1)
        param = np.ascontiguousarray(param, dtype=np.float64)
        if param.shape != (len(kind), OBSTACLE_PARAMS):
            raise ValueError(f"param must have shape ({len(kind)}, {OBSTACLE_PARAMS}), one row per primitive, got {param.shape}")
        check(lib.dexr_obstacle_set_create(len(kind), _ptr(kind, C.c_int32), _ptr(param, C.c_double), C.byref(self._h)))
        n = C.c_int32()
        check(lib.dexr_obstacle_set_info(self._h, C.byref(n)))
        self.n_prim = int(n.value)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib is not None:
            _lib.dexr_obstacle_set_destroy(h)
            self._h = None

    @property
    def handle(self) -> C.c_void_p:
        return self._h


class SdfGrid:
    """Owns one dexr_sdf_grid (include/dexr_sdf_grid.h): float32 samples values (nx, ny, nz) of a signed-distance field in C order,
    resident in HBM; sample (ix, iy, iz) sits at origin + (ix, iy, iz) * spacing of the obstacle frame.  Any SphereModel's grid_*
    methods take it."""

    def __init__(self, values, origin, spacing):
        lib = load()
        self._h = C.c_void_p()
        values = np.ascontiguousarray(values, dtype=np.float32)
        origin = np.ascontiguousarray(origin, dtype=np.float64).reshape(-1)
        spacing = np.ascontiguousarray(spacing, dtype=np.float64).reshape(-1)
        if values.ndim != 3 or origin.shape != (3,) or spacing.shape != (3,):
            raise ValueError(f"values must have shape (nx, ny, nz), origin and spacing (3,), got {values.shape}, {origin.shape}, {spacing.shape}")
        n = np.array(values.shape, dtype=np.int32)
        check(lib.dexr_sdf_grid_create(_ptr(n, C.c_int32), _ptr(origin, C.c_double), _ptr(spacing, C.c_double), _ptr(values, C.c_float),
                                       C.byref(self._h)))
        check(lib.dexr_sdf_grid_info(self._h, _ptr(n, C.c_int32), None, None))
        self.shape = tuple(int(v) for v in n)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib is not None:
            _lib.dexr_sdf_grid_destroy(h)
            self._h = None

    @property
    def handle(self) -> C.c_void_p:
        return self._h


class DeviceSdfGrid(SdfGrid):
    """Owns one dexr_sdf_grid made by dexr_sdf_grid_create_dev (include/dexr_sdf_grid_dev.h): the samples are allocated on the current
    device and set, on `stream`, to zero or to a device-to-device copy of the n[0] n[1] n[2] float32 at values_ptr.  A producer
    writes them through `values_ptr`; keeping them finite is the producer's contract.  Everything that takes an SdfGrid takes it."""

    def __init__(self, n, origin, spacing, values_ptr: int = 0, stream: int = 0):
        lib = load()
        self._h = C.c_void_p()
        n, origin, spacing = TriangleMesh._grid_args(n, origin, spacing)
        check(lib.dexr_sdf_grid_create_dev(_ptr(n, C.c_int32), _ptr(origin, C.c_double), _ptr(spacing, C.c_double), values_ptr or None,
                                           stream or None, C.byref(self._h)))
        self.shape = tuple(int(v) for v in n)

    @property
    def values_ptr(self) -> int:
        """the device address of the samples (dexr_sdf_grid_values_dev)"""
        return int(load().dexr_sdf_grid_values_dev(self._h) or 0)

    def download(self, stream: int = 0) -> np.ndarray:
        """-> the samples (nx, ny, nz) float32 on the host, as they are after everything enqueued on `stream` before this call; it
        synchronises that stream (dexr_sdf_grid_download)."""
        values = np.zeros(self.shape, dtype=np.float32)
        check(load().dexr_sdf_grid_download(self._h, _ptr(values, C.c_float), stream or None))
        return values


def _edt_grid_args(n, origin=None):
    n = np.ascontiguousarray(n, dtype=np.int32).reshape(-1)
    if n.shape != (3,):
        raise ValueError(f"n must have shape (3,), got {n.shape}")
    if origin is None:
        return n
    origin = np.ascontiguousarray(origin, dtype=np.float64).reshape(-1)
    if origin.shape != (3,):
        raise ValueError(f"origin must have shape (3,), got {origin.shape}")
    return n, origin


def edt_workspace_bytes(n) -> int:
    """bytes of device workspace a distance transform on a grid of n (3,) samples needs (dexr_edt_workspace_bytes)"""
    n = _edt_grid_args(n)
    out = C.c_size_t(0)
    check(load().dexr_edt_workspace_bytes(_ptr(n, C.c_int32), C.byref(out)))
    return int(out.value)


def edt_points_dev(points_ptr: int, N: int, n, origin, h: float, min_points: int, radius: float, max_distance: float, values_ptr: int,
                   d2_ptr: int = 0, count_ptr: int = 0, workspace_ptr: int = 0, workspace_bytes: int = 0, stream: int = 0):
    """device pointers (include/dexr_distance_transform.h): points (N, 3) float32 -> values (n) float32, d2 and count (n) int32 or 0.
    n and origin are host arrays.  Never synchronises, never allocates."""
    n, origin = _edt_grid_args(n, origin)
    check(load().dexr_edt_points_dev(points_ptr or None, int(N), _ptr(n, C.c_int32), _ptr(origin, C.c_double), float(h), int(min_points),
                                     float(radius), float(max_distance), values_ptr or None, d2_ptr or None, count_ptr or None,
                                     workspace_ptr or None, int(workspace_bytes), stream or None))


def edt_occupancy_dev(occ_ptr: int, n, h: float, signed: bool, radius: float, max_distance: float, values_ptr: int, d2_ptr: int = 0,
                      workspace_ptr: int = 0, workspace_bytes: int = 0, stream: int = 0):
    """device pointers: occ (n) uint8 -> values (n) float32, d2 (n) int32 or 0 (dexr_edt_occupancy_dev).  Never synchronises, never
    allocates."""
    n = _edt_grid_args(n)
    check(load().dexr_edt_occupancy_dev(occ_ptr or None, _ptr(n, C.c_int32), float(h), int(bool(signed)), float(radius), float(max_distance),
                                        values_ptr or None, d2_ptr or None, workspace_ptr or None, int(workspace_bytes), stream or None))


def _edt_host_outputs(n):
    ok = n.min() >= SDF_GRID_MIN_DIM and n.max() <= SDF_GRID_MAX_DIM and int(n[0]) * int(n[1]) * int(n[2]) <= SDF_GRID_MAX_SAMPLES
    shape = tuple(int(k) for k in n) if ok else (1,)  # (a refused shape: the library says why)
    return np.zeros(shape, dtype=np.float32), np.zeros(shape, dtype=np.int32)


def edt_points(points, n, origin, h: float, min_points: int = 1, radius: float = 0.0, max_distance: float = 1.0):
    """points (N, 3) float32 on the host -> values float32, d2 int32, count int32, each (n) (dexr_edt_points)."""
    points = np.ascontiguousarray(points, dtype=np.float32)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"points must have shape (N, 3), got {points.shape}")
    n, origin = _edt_grid_args(n, origin)
    values, d2 = _edt_host_outputs(n)
    count = np.zeros_like(d2)
    check(load().dexr_edt_points(_ptr(points, C.c_float) if len(points) else None, len(points), _ptr(n, C.c_int32), _ptr(origin, C.c_double),
                                 float(h), int(min_points), float(radius), float(max_distance), _ptr(values, C.c_float), _ptr(d2, C.c_int32),
                                 _ptr(count, C.c_int32)))
    return values, d2, count


def edt_occupancy(occ, h: float, signed: bool = True, radius: float = 0.0, max_distance: float = 1.0):
    """occ (nx, ny, nz) uint8 on the host -> values float32, d2 int32 (to the occupied voxels), each of occ's shape
    (dexr_edt_occupancy)."""
    occ = np.ascontiguousarray(occ, dtype=np.uint8)
    if occ.ndim != 3:
        raise ValueError(f"occ must have shape (nx, ny, nz), got {occ.shape}")
    n = np.array(occ.shape, dtype=np.int32)
    values, d2 = _edt_host_outputs(n)
    check(load().dexr_edt_occupancy(_ptr(occ, C.c_uint8), _ptr(n, C.c_int32), float(h), int(bool(signed)), float(radius), float(max_distance),
                                    _ptr(values, C.c_float), _ptr(d2, C.c_int32)))
    return values, d2


def mesh_points_per_launch(n_triangle: int) -> int:
    """points of one launch of the mesh kernels against a mesh of n_triangle triangles (include/dexr_mesh_sdf.h, BOUNDED LAUNCHES)"""
    return max(1, (MESH_PAIRS_PER_LAUNCH // n_triangle) // MESH_BLOCK_POINTS) * MESH_BLOCK_POINTS


class TriangleMesh:
    """Owns one dexr_mesh (include/dexr_mesh_sdf.h): vertices (V, 3) float64 and faces (T, 3) int32, the per-triangle records
    resident in HBM in float32 and float64.  Signed distances (the sign from the generalised winding number) of points or of the
    samples of a regular grid, brute force: points x T pairs."""

    def __init__(self, vertices, faces):
        lib = load()
        self._h = C.c_void_p()
        vertices = np.ascontiguousarray(vertices, dtype=np.float64)
        faces = np.ascontiguousarray(faces, dtype=np.int32)
        if vertices.ndim != 2 or vertices.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3:
            raise ValueError(f"vertices must have shape (V, 3) and faces (T, 3), got {vertices.shape}, {faces.shape}")
        check(lib.dexr_mesh_create(len(vertices), _ptr(vertices, C.c_double), len(faces), _ptr(faces, C.c_int32), C.byref(self._h)))
        nv, nt = C.c_int32(), C.c_int32()
        bounds = np.zeros(6, dtype=np.float64)
        check(lib.dexr_mesh_info(self._h, C.byref(nv), C.byref(nt), _ptr(bounds, C.c_double)))
        self.n_vertex, self.n_triangle, self.bounds = int(nv.value), int(nt.value), bounds.reshape(2, 3)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib is not None:
            _lib.dexr_mesh_destroy(h)
            self._h = None

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    @staticmethod
    def _grid_args(n, origin, spacing):
        n = np.ascontiguousarray(n, dtype=np.int32).reshape(-1)
        origin = np.ascontiguousarray(origin, dtype=np.float64).reshape(-1)
        spacing = np.ascontiguousarray(spacing, dtype=np.float64).reshape(-1)
        if n.shape != (3,) or origin.shape != (3,) or spacing.shape != (3,):
            raise ValueError(f"n, origin and spacing must each have shape (3,), got {n.shape}, {origin.shape}, {spacing.shape}")
        return n, origin, spacing

    def distances_dev(self, P: int, points_ptr: int, dist_ptr: int, winding_ptr: int = 0, stream: int = 0):
        """device pointers, float32: points (P, 3) -> dist (P), winding (P) or 0.  Never synchronises, never allocates."""
        check(load().dexr_mesh_distances_dev(self._h, P, points_ptr or None, dist_ptr or None, winding_ptr or None, stream or None))

    def distances(self, points, winding: bool = False):
        """points (P, 3) float64 on the host -> dist (P) float64 [, winding (P) float64], float64 arithmetic on the device."""
        points = np.ascontiguousarray(points, dtype=np.float64)
        if points.ndim != 2 or points.shape[1] != 3:
            raise ValueError(f"points must have shape (P, 3), got {points.shape}")
        P = points.shape[0]
        dist = np.zeros(P, dtype=np.float64)
        wind = np.zeros(P, dtype=np.float64) if winding else None
        check(load().dexr_mesh_distances(self._h, P, _ptr(points, C.c_double), _ptr(dist, C.c_double), _ptr(wind, C.c_double)))
        return (dist, wind) if winding else dist

    def sample_grid_dev(self, n, origin, spacing, values_ptr: int, stream: int = 0):
        """values (n[0], n[1], n[2]) float32 on the device, float32 arithmetic.  Never synchronises, never allocates."""
        n, origin, spacing = self._grid_args(n, origin, spacing)
        check(load().dexr_mesh_sample_grid_dev(self._h, _ptr(n, C.c_int32), _ptr(origin, C.c_double), _ptr(spacing, C.c_double),
                                               values_ptr or None, stream or None))

    def sample_grid(self, n, origin, spacing):
        """-> values (n[0], n[1], n[2]) float32 on the host: float64 arithmetic on the device, rounded to float32 at the store."""
        n, origin, spacing = self._grid_args(n, origin, spacing)
        lo, hi = SDF_GRID_MIN_DIM, SDF_GRID_MAX_DIM
        ok = n.min() >= lo and n.max() <= hi and int(n[0]) * int(n[1]) * int(n[2]) <= SDF_GRID_MAX_SAMPLES
        values = np.zeros(tuple(int(k) for k in n) if ok else (1,), dtype=np.float32)  # (a refused shape: the library says why)
        check(load().dexr_mesh_sample_grid(self._h, _ptr(n, C.c_int32), _ptr(origin, C.c_double), _ptr(spacing, C.c_double),
                                           _ptr(values, C.c_float)))
        return values


def _sphere_fit_args(dims, spacing, offset, k):
    dims = np.ascontiguousarray(dims, dtype=np.int32)
    if dims.ndim != 2 or dims.shape[1] != 3:
        raise ValueError(f"dims must have shape (n_body, 3), got {dims.shape}")
    n_body = dims.shape[0]
    spacing = np.ascontiguousarray(spacing, dtype=np.float64).reshape(-1)
    offset = np.ascontiguousarray(offset, dtype=np.int64).reshape(-1)
    k = np.ascontiguousarray(k, dtype=np.int32).reshape(-1)
    if spacing.shape != (n_body,) or offset.shape != (n_body,) or k.shape != (n_body,):
        raise ValueError(f"spacing, offset and k must each have shape ({n_body},), got {spacing.shape}, {offset.shape}, {k.shape}")
    return n_body, dims, spacing, offset, k


def sphere_fit_workspace_bytes(dims) -> int:
    """bytes of device workspace a sphere fit of bodies of dims (n_body, 3) needs (dexr_sphere_fit_workspace_bytes)"""
    dims = np.ascontiguousarray(dims, dtype=np.int32)
    if dims.ndim != 2 or dims.shape[1] != 3:
        raise ValueError(f"dims must have shape (n_body, 3), got {dims.shape}")
    n = int(load().dexr_sphere_fit_workspace_bytes(dims.shape[0], _ptr(dims, C.c_int32)))
    if n == 0:
        raise DexrError(f"libdexr error -1: {load().dexr_last_error().decode()}")
    return n


def sphere_fit_dev(dims, spacing, offset, k, min_radius: float, inflate: float, coverage: float, n_values: int, values_ptr: int, index_ptr: int,
                   gain_ptr: int, count_ptr: int, workspace_ptr: int, workspace_bytes: int, stream: int = 0):
    """device pointers (include/dexr_sphere_fit.h): values (n_values) float32 -> index, gain (n_body, max k) and count (n_body, 3)
    int32.  dims, spacing, offset and k are host arrays.  Never synchronises, never allocates."""
    n_body, dims, spacing, offset, k = _sphere_fit_args(dims, spacing, offset, k)
    check(load().dexr_sphere_fit_dev(n_body, _ptr(dims, C.c_int32), _ptr(spacing, C.c_double), _ptr(offset, C.c_int64), _ptr(k, C.c_int32),
                                     float(min_radius), float(inflate), float(coverage), int(n_values), values_ptr or None, index_ptr or None,
                                     gain_ptr or None, count_ptr or None, workspace_ptr or None, int(workspace_bytes), stream or None))


def sphere_fit(dims, spacing, offset, k, min_radius: float, inflate: float, coverage: float, values):
    """values (n_values) float32 on the host -> index, gain (n_body, max k) and count (n_body, 3) int32 (dexr_sphere_fit)."""
    n_body, dims, spacing, offset, k = _sphere_fit_args(dims, spacing, offset, k)
    values = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    k_max = int(k.max()) if n_body and 1 <= int(k.max()) <= SPHERE_MAX else 1  # (a refused k: the library says why)
    index = np.zeros((n_body, k_max), dtype=np.int32)
    gain = np.zeros((n_body, k_max), dtype=np.int32)
    count = np.zeros((n_body, 3), dtype=np.int32)
    check(load().dexr_sphere_fit(n_body, _ptr(dims, C.c_int32), _ptr(spacing, C.c_double), _ptr(offset, C.c_int64), _ptr(k, C.c_int32),
                                 float(min_radius), float(inflate), float(coverage), values.size, _ptr(values, C.c_float),
                                 _ptr(index, C.c_int32), _ptr(gain, C.c_int32), _ptr(count, C.c_int32)))
    return index, gain, count


def seq_compose_dev(B: int, T: int, dof_kind, dof_idx, dof_mult, dof_off, n_opt: int, n_fixed: int, qraw_ptr: int,
                    fixed_ptr: int, alpha: float, filter_ptr: int, first_frame_initialises: bool, out_ptr: int,
                    stream: int = 0):
    """robot-qpos composition + mimic fill + low-pass filter for T x B frames (dexr_seq_compose_dev)."""
    kind = np.ascontiguousarray(dof_kind, dtype=np.int32)
    idx = np.ascontiguousarray(dof_idx, dtype=np.int32)
    mult = np.ascontiguousarray(dof_mult, dtype=np.float64)
    off = np.ascontiguousarray(dof_off, dtype=np.float64)
    check(load().dexr_seq_compose_dev(B, T, len(kind), n_opt, n_fixed, _ptr(kind, C.c_int32), _ptr(idx, C.c_int32),
                                      _ptr(mult, C.c_double), _ptr(off, C.c_double), qraw_ptr or None, fixed_ptr or None,
                                      float(alpha), filter_ptr or None, 1 if first_frame_initialises else 0,
                                      out_ptr or None, stream or None))


def fleet_workspace_bytes(B: int) -> int:
    return int(load().dexr_fleet_workspace_bytes(B))


def retarget_multi_dev(models, B: int, model_id_ptr: int, kp_ptr: int, last_ptr: int, ld: int, state_ptr: int,
                       q_ptr: int, status_ptr: int, ws_ptr: int, ws_bytes: int, opts: Optional[SolveOptions] = None,
                       stream: int = 0, fixed_ptr: int = 0, ld_fixed: int = 0):
    """Mixed-fleet batch (dexr_retarget_multi_dev): `models` is a list of Model handles; `fixed_ptr` addresses (B, ld_fixed)
    float32 rows of caller-supplied fixed-joint values (0: no model has any)."""
    arr = (C.c_void_p * len(models))(*[m.handle for m in models])
    check(load().dexr_retarget_multi_dev(arr, len(models), B, model_id_ptr or None, kp_ptr or None, fixed_ptr or None, ld_fixed,
                                         last_ptr or None, ld,
                                         state_ptr or None, q_ptr or None, status_ptr or None,
                                         C.byref(opts) if opts is not None else None, ws_ptr or None, ws_bytes,
                                         stream or None))


def retarget_multi(models, model_id: np.ndarray, keypoints: np.ndarray, last: np.ndarray, state: Optional[np.ndarray] = None,
                   qpos_out: Optional[np.ndarray] = None, opts: Optional[SolveOptions] = None, want_status: bool = False,
                   fixed: Optional[np.ndarray] = None):
    """Mixed-fleet batch on HOST arrays (dexr_retarget_multi): model_id (B,) int32, keypoints (B,21,3) f32, last (B,ld) f32,
    state (B,) uint32 in/out or None.  Returns qpos (B,ld) f32 [, status (B,) int32]; `qpos_out` (in-out) supplies the
    values of the rows / columns the call leaves untouched (default zeros)."""
    mid = np.ascontiguousarray(model_id, dtype=np.int32)
    kp = np.ascontiguousarray(keypoints, dtype=np.float32)
    la = np.ascontiguousarray(last, dtype=np.float32)
    B, ld = la.shape
    if kp.shape != (B, 21, 3) or mid.shape != (B,):
        raise ValueError(f"model_id must be ({B},), keypoints ({B}, 21, 3)")
    q = np.zeros((B, ld), np.float32) if qpos_out is None else np.ascontiguousarray(qpos_out, dtype=np.float32)
    if q.shape != (B, ld):
        raise ValueError(f"qpos_out must have shape ({B}, {ld})")
    if state is not None and (state.dtype != np.uint32 or state.shape != (B,) or not state.flags["C_CONTIGUOUS"]):
        raise ValueError(f"state must be a C-contiguous uint32 array of shape ({B},)")
    status = np.zeros(B, np.int32)
    fx = None if fixed is None else np.ascontiguousarray(fixed, dtype=np.float32).reshape(B, -1)
    arr = (C.c_void_p * len(models))(*[m.handle for m in models])
    check(load().dexr_retarget_multi(arr, len(models), B, _ptr(mid, C.c_int32), _ptr(kp, C.c_float), _ptr(fx, C.c_float),
                                     0 if fx is None else fx.shape[1], _ptr(la, C.c_float), ld,
                                     _ptr(state, C.c_uint32), _ptr(q, C.c_float), _ptr(status, C.c_int32),
                                     C.byref(opts) if opts is not None else None))
    return (q, status) if want_status else q


def comm_unique_id() -> bytes:
    """Rank 0: the RCCL unique id every rank of a communicator has to be handed (dexr_comm_unique_id)."""
    buf = C.create_string_buffer(UNIQUE_ID_BYTES)
    check(load().dexr_comm_unique_id(buf))
    return buf.raw


class Comm:
    """Owns one dexr_comm: an RCCL communicator bound to the current HIP device (collective constructor)."""

    def __init__(self, unique_id: bytes, rank: int, world: int):
        if len(unique_id) != UNIQUE_ID_BYTES:
            raise ValueError(f"unique id must be {UNIQUE_ID_BYTES} bytes")
        self._h = C.c_void_p()
        buf = C.create_string_buffer(unique_id, UNIQUE_ID_BYTES)
        check(load().dexr_comm_create(buf, rank, world, C.byref(self._h)))
        self.rank, self.world = rank, world

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib is not None:
            _lib.dexr_comm_destroy(h)
            self._h = None

    __del__ = close

    def rccl_version(self) -> int:
        v = C.c_int32()
        check(load().dexr_comm_info(self._h, None, None, C.byref(v)))
        return int(v.value)

    def allgather(self, send_ptr: int, recv_ptr: int, bytes_per_rank: int, stream: int = 0):
        """recv[r] = rank r's send block; device addresses; enqueued on `stream` (no synchronisation)."""
        check(load().dexr_allgather(self._h, send_ptr or None, recv_ptr or None, bytes_per_rank, stream or None))

    def max_f64(self, values, stream: int = 0) -> np.ndarray:
        v = np.ascontiguousarray(values, dtype=np.float64).copy()
        check(load().dexr_comm_max_f64(self._h, _ptr(v, C.c_double), len(v), stream or None))
        return v

    def barrier(self, stream: int = 0):
        check(load().dexr_comm_barrier(self._h, stream or None))
