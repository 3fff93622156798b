"""The reference's online benchmark shape, run against the drop-in under the reference's package name: `dex_retargeting` (and
every `dex_retargeting.<module>`) is aliased to `dex_retargeting_amd` in sys.modules, then 7 robots x {vector, DexPilot} are
each built from their default right-hand config and fed the 621-frame human fixture (tests/golden/human_joint_right_f32.npy),
ONE SeqRetargeting.retarget(ref_value) call per frame with only the call inside the timer.  One row per robot and kind:
summed seconds and fps = 621 / seconds.

    python tests/reference_suite/run_profile_script.py            # one text line per row
    python tests/reference_suite/run_profile_script.py --json     # + one JSON line: {"rows": [{"kind", "robot", "seconds", "fps"} x 14]}
    python tests/reference_suite/run_profile_script.py --json --passes 2   # the 14 rows twice in one process (second: warm HIP context)

bench.py --full runs this file in a process of its own (DETAIL line `reference_profile_script`); tests/reference_suite/
test_reference_profile_script.py runs it on the GPU and checks the 14 rows."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

HUMAN_FIXTURE = os.path.join(REPO, "tests", "golden", "human_joint_right_f32.npy")
MARKER = "ONLINE_PROFILE_ROWS "


def alias_package() -> None:
    import importlib
    import pkgutil

    import dex_retargeting_amd as pkg

    sys.modules["dex_retargeting"] = pkg
    for m in pkgutil.iter_modules(pkg.__path__):
        if m.name.startswith("_") or m.ispkg or not os.path.exists(os.path.join(pkg.__path__[0], m.name + ".py")):
            continue
        sys.modules[f"dex_retargeting.{m.name}"] = importlib.import_module(f"dex_retargeting_amd.{m.name}")


def profile_row(robot_name, retargeting_type, data):
    """Seconds spent inside SeqRetargeting.retarget over every fixture frame, for one robot and retargeting type."""
    from dex_retargeting.constants import HandType, get_default_config_path
    from dex_retargeting.retargeting_config import RetargetingConfig

    path = get_default_config_path(robot_name, retargeting_type, HandType.right)
    retargeting = RetargetingConfig.load_from_file(path).build()
    indices = retargeting.optimizer.target_link_human_indices
    total = 0.0
    for joint_pos in data:
        ref_value = joint_pos[indices[1, :], :] - joint_pos[indices[0, :], :]
        tic = time.perf_counter()
        retargeting.retarget(ref_value)
        total += time.perf_counter() - tic
    return total


def run():
    """-> (text lines, rows): 7 vector rows, then 7 DexPilot rows, in RobotName order."""
    alias_package()
    from dex_retargeting.constants import DEFAULT_URDF_DIR, ROBOT_NAME_MAP, RobotName, RetargetingType
    from dex_retargeting.retargeting_config import RetargetingConfig

    RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
    data = np.load(HUMAN_FIXTURE).astype(np.float64)
    lines, rows = [f"online retargeting profile: {len(data)} hand poses per robot"], []
    for kind in (RetargetingType.vector, RetargetingType.dexpilot):
        for robot_name in RobotName:
            seconds = profile_row(robot_name, kind, data)
            fps = len(data) / seconds
            rows.append({"kind": kind.name, "robot": ROBOT_NAME_MAP[robot_name], "seconds": seconds, "fps": fps})
            lines.append(f"{kind.name} {ROBOT_NAME_MAP[robot_name]}: {seconds:.4f} s, {fps:.1f} fps")
    return lines, rows


if __name__ == "__main__":
    passes = int(sys.argv[sys.argv.index("--passes") + 1]) if "--passes" in sys.argv else 1
    for p in range(passes):  # (pass 1 pays the process's first HIP context inside its first row; pass 2: a warm process)
        lines, rows = run()
        print("\n".join(lines))
        if "--json" in sys.argv:
            print(MARKER + json.dumps({"pass": p + 1, "frames": len(np.load(HUMAN_FIXTURE)), "rows": rows}))
        sys.stdout.flush()
