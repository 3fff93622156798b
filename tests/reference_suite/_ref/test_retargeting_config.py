"""Config parsing through the drop-in under the reference's package name (`dex_retargeting`, aliased by ../conftest.py).

Every shipped vector / position / DexPilot config builds a SeqRetargeting from its file; config mappings given as dicts
build the same objects as the files they came from; `add_dummy_free_joint` puts six dummy free joints in front of the
robot's own.  The configs are read through the layout the reference's tests use (<suite>/src/dex_retargeting/configs
and <suite>/assets/robots/hands, committed links to the package's own files)."""
from pathlib import Path

import numpy as np
import pytest
import yaml

from dex_retargeting.retargeting_config import RetargetingConfig
from dex_retargeting.seq_retarget import SeqRetargeting

SUITE = Path(__file__).resolve().parent.parent
CONFIG_DIR = SUITE / "src" / "dex_retargeting" / "configs"
URDF_DIR = SUITE / "assets" / "robots" / "hands"

VECTOR = ["teleop/allegro_hand_right.yml", "teleop/allegro_hand_left.yml", "teleop/shadow_hand_right.yml",
          "teleop/schunk_svh_hand_right.yml", "teleop/leap_hand_right.yml", "teleop/ability_hand_right.yml",
          "teleop/ability_hand_left.yml"]
POSITION = ["offline/allegro_hand_right.yml", "offline/shadow_hand_right.yml", "offline/schunk_svh_hand_right.yml",
            "offline/leap_hand_right.yml", "offline/ability_hand_right.yml"]
DEXPILOT = ["teleop/allegro_hand_right_dexpilot.yml", "teleop/allegro_hand_left_dexpilot.yml",
            "teleop/shadow_hand_right_dexpilot.yml", "teleop/schunk_svh_hand_right_dexpilot.yml",
            "teleop/leap_hand_right_dexpilot.yml"]


def _mapping(rel):
    with open(CONFIG_DIR / rel) as f:
        return yaml.safe_load(f)["retargeting"]


def _check_built(seq, kind):
    opt = seq.optimizer
    assert isinstance(seq, SeqRetargeting)
    assert opt.retargeting_type == kind.upper()
    assert seq.joint_limits.shape == (opt.opt_dof, 2)
    assert np.all(seq.joint_limits[:, 0] <= seq.joint_limits[:, 1])
    assert set(opt.target_joint_names) <= set(opt.robot.dof_joint_names)


class TestRetargetingConfig:
    RetargetingConfig.set_default_urdf_dir(str(URDF_DIR))

    @pytest.mark.parametrize("config_path", VECTOR + POSITION + DEXPILOT)
    def test_path_config_parsing(self, config_path):
        seq = RetargetingConfig.load_from_file(CONFIG_DIR / config_path).build()
        _check_built(seq, _mapping(config_path)["type"])

    def test_dict_config_parsing(self):
        rel = "offline/ability_hand_right.yml"
        from_dict = RetargetingConfig.from_dict(_mapping(rel), {"low_pass_alpha": 1}).build()
        from_file = RetargetingConfig.load_from_file(CONFIG_DIR / rel).build()
        _check_built(from_dict, "position")
        assert from_dict.optimizer.target_joint_names == from_file.optimizer.target_joint_names
        np.testing.assert_array_equal(from_dict.joint_limits, from_file.joint_limits)

    def test_multi_dict_config_parsing(self):
        rels = ["teleop/allegro_hand_right.yml", "teleop/leap_hand_right_dexpilot.yml"]
        seqs = [RetargetingConfig.from_dict(_mapping(r)).build() for r in rels]
        for seq, rel in zip(seqs, rels):
            _check_built(seq, _mapping(rel)["type"])
        assert seqs[0].optimizer.robot is not seqs[1].optimizer.robot
        assert seqs[0].optimizer.robot.dof_joint_names != seqs[1].optimizer.robot.dof_joint_names

    @pytest.mark.parametrize("config_path", POSITION)
    def test_add_dummy_joint(self, config_path):
        plain = RetargetingConfig.load_from_file(CONFIG_DIR / config_path, {"add_dummy_free_joint": False}).build()
        dummy = RetargetingConfig.load_from_file(CONFIG_DIR / config_path, {"add_dummy_free_joint": True}).build()
        n_robot, n_active = plain.optimizer.robot.dof, len(plain.optimizer.target_joint_names)
        assert dummy.optimizer.robot.dof == n_robot + 6
        assert dummy.joint_limits.shape == (n_active + 6, 2)
        assert all("dummy" in name for name in dummy.optimizer.robot.dof_joint_names[:6])
        assert dummy.optimizer.robot.dof_joint_names[6:] == plain.optimizer.robot.dof_joint_names
