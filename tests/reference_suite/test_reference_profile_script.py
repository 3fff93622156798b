"""GPU: the reference's online benchmark shape against the drop-in (run_profile_script.py, in a process of its own):
7 robots x {vector, DexPilot} = 14 "fps" rows over the 621-frame fixture, one SeqRetargeting.retarget per frame."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
ROBOTS = ["allegro_hand", "shadow_hand", "schunk_svh_hand", "leap_hand", "ability_hand", "inspire_hand", "panda_gripper"]


@pytest.mark.gpu
def test_online_profile_rows_against_the_drop_in():
    r = subprocess.run([sys.executable, os.path.join(HERE, "run_profile_script.py"), "--json"], capture_output=True, text=True,
                       timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    rec = json.loads([l for l in lines if l.startswith("ONLINE_PROFILE_ROWS ")][0].split(" ", 1)[1])
    assert rec["frames"] == 621
    rows = rec["rows"]
    assert [(x["kind"], x["robot"]) for x in rows] == [("vector", n) for n in ROBOTS] + [("dexpilot", n) for n in ROBOTS]
    for x in rows:
        assert x["fps"] > 0 and abs(x["fps"] * x["seconds"] - 621) < 1e-6 * 621
