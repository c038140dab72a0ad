"""CPU-only checks: the C-ABI library loads and exports every symbol include/parc_hip.h declares, and the
host-side logic (MJCF parser, ray template, config -> observation layout, motion file reader) matches the
reference's golden data.  No compute call is made without a GPU."""
import json
import os
import pickle
import re

import numpy as np
import pytest
import torch

from conftest import REPO, golden


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as ge
    ge.build()
    from parc_amd import _hip
    L = _hip.lib()
    hdr = open(os.path.join(REPO, "include", "parc_hip.h")).read()
    hdr_sim = os.path.join(REPO, "include", "parc_sim.h")
    if os.path.exists(hdr_sim):
        hdr += open(hdr_sim).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(parc_[a-z0-9_]+)\s*\(", hdr, flags=re.M))
    assert len(declared) >= 45 and "parc_moments_workspace_floats" in declared and "parc_sim_step" in declared
    for name in declared:
        assert hasattr(L, name), "missing export " + name
    assert L.parc_abi_version() == 1
    # ... and INTEGRATION.md says, for every one of them, which piece of the reference it stands for
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert not [n for n in sorted(declared) if n not in doc]


def test_product_library_carries_no_diagnostics():
    """The timing-ablation bits of parc_track_post_step, the heightmap kernel's measurement knobs and the reference simulator kernel
    live in the diagnostics library only (tools/parc_diag.py, -DPARC_DIAG_BUILD): the product library answers PARC_EINVAL (-1) to any
    bit of `what` outside PARC_POST_ALL - before any HIP call, so this runs without a GPU - and exports none of those symbols; no
    environment variable reaches a launch (PARC_POST_DIAG / PARC_ALLOW_STALE_LIB are gone)."""
    import subprocess
    import __graft_entry__ as ge
    ge.build()
    from parc_amd import _hip
    from parc_amd.anim.kin_char_model import KinCharModel
    from parc_amd.assets import humanoid_spec
    L = _hip.lib()
    km = KinCharModel("cpu")
    km.load_char_file(humanoid_spec.write_mjcf())
    ms = _hip.MotionLibS()
    ms.num_bodies, ms.dof_size = 15, 28
    full = _hip.POST_OBS | _hip.POST_REWARD_DONE | _hip.POST_HF | _hip.POST_TARGETS
    for bit in (0x100, 0x10000, 0x80000, 0x100000, 0x200000, 0x1000000, 1 << 30):
        rc = L.parc_track_post_step(None, km.c_struct(), ms, _hip.TerrainS(), _hip.TrackCfgS(), _hip.EnvBuffersS(), None, 0, full | bit, None)
        assert rc == -1, (hex(bit), rc)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _hip.LIB_PATH], text=True)
    assert "parc_track_post_step" in syms
    for forbidden in ("parc_tune_", "parc_diag_", "sim_step_kernel"):
        assert forbidden not in syms.replace("sim_step_bpl_kernel", ""), forbidden
    dsyms = subprocess.check_output(["nm", "-D", "--defined-only", _hip.DIAG_LIB_PATH], text=True)
    for needed in ("parc_tune_hf_ablation", "parc_tune_hf_groups", "parc_tune_hf_envs_per_block", "parc_diag_sim_step_env_per_lane"):
        assert needed in dsyms, needed
    hdr = open(os.path.join(REPO, "tools", "parc_diag.h")).read()
    for name in set(re.findall(r"\bint\s+(parc_[a-z0-9_]+)\s*\(", hdr)):
        assert name in dsyms, name
    for src in ("parc_amd/tracker_core.py", "parc_amd/_hip.py"):
        text = open(os.path.join(REPO, src)).read()
        assert "PARC_POST_DIAG" not in text and "PARC_ALLOW_STALE_LIB" not in text and "environ.get(\"PARC_POST" not in text


def test_only_the_checkers_touch_the_oracle():
    """oracle/ is test infrastructure: nothing of the package, of tools/ or of the driver entry points imports it - only tests/ (with
    tests/tools/), smoke_impl.py (smoke()'s check) and the cpu_baseline leg of bench.py do."""
    import ast
    import glob
    offenders = []
    files = glob.glob(os.path.join(REPO, "parc_amd", "**", "*.py"), recursive=True) + glob.glob(os.path.join(REPO, "tools", "**", "*.py"), recursive=True) \
        + [os.path.join(REPO, "__graft_entry__.py"), os.path.join(REPO, "bench.py")]
    assert len(files) > 60
    for f in files:
        tree = ast.parse(open(f).read())
        for fn_name, node in [(None, n) for n in tree.body] + [(fn.name, n) for fn in ast.walk(tree) if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef))
                                                              for n in ast.walk(fn)]:
            mods = []
            if isinstance(node, ast.Import):
                mods = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom) and node.level == 0:
                mods = [node.module or ""]
            if any(m == "oracle" or m.startswith("oracle.") for m in mods):
                if not (os.path.basename(f) == "bench.py" and fn_name == "cpu_baseline"):
                    offenders.append((os.path.relpath(f, REPO), fn_name))
    assert not offenders, offenders
    for f in glob.glob(os.path.join(REPO, "parc_amd", "**", "*.py"), recursive=True):
        text = open(f).read()
        assert "liboracle" not in text and "parc_oracle" not in text and "sim_host" not in text, f


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Error behaviour of the C ABI (include/parc_hip.h: 0 ok, PARC_EINVAL -1, PARC_EUNSUPPORTED -2): malformed calls of the rollout
    step's entry points are answered before any HIP call - so this runs without a GPU - instead of reaching a kernel with operands
    it would index out of bounds."""
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from parc_amd import _hip, _hip_sim  # noqa: F401  (_hip_sim declares the simulator's prototypes on the same handle)
    L = _hip.lib()
    cell = (ctypes.c_int64 * 2)()
    buf = (ctypes.c_float * 64)()
    a16 = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16          # a 16-byte aligned host address: never dereferenced
    P = ctypes.c_void_p
    EINVAL, EUNSUP = -1, -2
    # random numbers of a step: no state cell; a count below zero; an output count without its buffer; a tick without a modulus
    assert L.parc_rng_step(None, 1, None, P(a16), 4, None, 0, None, 0) == EINVAL
    assert L.parc_rng_step(None, 1, cell, P(a16), -4, None, 0, None, 0) == EINVAL
    assert L.parc_rng_step(None, 1, cell, None, 4, None, 0, None, 0) == EINVAL
    assert L.parc_rng_step(None, 1, cell, None, 0, None, 0, cell, 0) == EINVAL
    assert L.parc_rng_step(None, 1, cell, None, 0, None, 0, None, 0) == 0                   # nothing to draw, nothing to tick: a no-op
    # observation ingest: a width that is not a multiple of 4, a misaligned row pointer, a copy target without its row cell, sums
    # without their workspace
    ok = (None, 8, 8, P(a16), P(a16), P(a16), 5.0, P(a16))
    assert L.parc_obs_ingest(None, 8, 6, P(a16), P(a16), P(a16), 5.0, P(a16), None, None, None, None) == EINVAL
    assert L.parc_obs_ingest(None, 8, 8, P(a16 + 4), P(a16), P(a16), 5.0, P(a16), None, None, None, None) == EINVAL
    assert L.parc_obs_ingest(*ok, P(a16), None, None, None) == EINVAL
    assert L.parc_obs_ingest(*ok, None, None, P(a16), None) == EINVAL
    assert L.parc_obs_ingest(None, 0, 8, P(a16), P(a16), P(a16), 5.0, P(a16), None, None, None, None) == 0      # no rows: a no-op
    # action head + record: more action columns than its 32 lanes per env; a record target missing
    eight = [P(a16)] * 8
    assert L.parc_action_head_record(None, 4, 33, *eight, *([P(a16)] * 5), 45, cell) == EUNSUP
    assert L.parc_action_head_record(None, 4, 28, *eight, None, P(a16), P(a16), P(a16), P(a16), 45, cell) == EINVAL
    assert L.parc_action_head_record(None, 4, 28, *eight, *([P(a16)] * 5), 45, None) == EINVAL
    # row assembly: more rows than one grid dimension holds; no column map
    assert L.parc_assemble_obs(None, 70000, P(a16), 1312, None, None, P(a16), P(a16), 1314, None, 0) == EUNSUP
    assert L.parc_assemble_obs(None, 8, P(a16), 1312, None, None, None, P(a16), 1314, None, 0) == EINVAL
    # the simulator step that also advances the clock, without the clock
    assert L.parc_sim_step_tick(None, P(a16), _hip.TerrainS(), 4, *([P(a16)] * 8), 4, 1.0 / 120.0, None, None, 1.0 / 30.0) == EINVAL
    # timed post step without its events
    from parc_amd.anim.kin_char_model import KinCharModel
    from parc_amd.assets import humanoid_spec
    km = KinCharModel("cpu")
    km.load_char_file(humanoid_spec.write_mjcf())
    ms = _hip.MotionLibS()
    ms.num_bodies, ms.dof_size = 15, 28
    assert L.parc_track_post_step_timed(None, km.c_struct(), ms, _hip.TerrainS(), _hip.TrackCfgS(), _hip.EnvBuffersS(), None, 0,
                                        _hip.POST_OBS, None, None, None) == EINVAL


def test_g26_observation_layouts_and_the_shipped_configs():
    """The segment table IGParkourEnv._compute_obs(ret_obs_shapes=True) prints (fixture G26: the reference's own method, one entry per
    configuration variant) against TrackerConfig.obs_layout, with the gather map checked on a numbered row; and the two env
    configurations the reference SHIPS - data/envs/ig_parkour_env.yaml (motion-generator env, has_target_xy_obs, replan timer) and
    data/terrains/dm_env_civilization.yaml - parsed by the reference's yaml and accepted as they are."""
    from parc_amd.anim.kin_char_model import KinCharModel
    from parc_amd.assets import humanoid_spec
    from parc_amd.envs.ig_parkour.default_config import default_env_config
    from parc_amd.tracker_core import TrackerConfig
    g = json.load(open(os.path.join(REPO, "tests", "golden", "g26_obs_variants.json")))
    km = KinCharModel("cpu")
    km.load_char_file(humanoid_spec.write_mjcf())
    for tag, table in g["variants"].items():
        over = {k: v for k, v in table["config"].items() if not k.startswith("_") and k != "enable_replan_timer_obs"}
        cfg = TrackerConfig(dict(default_env_config()["env"], **over), km, 441)
        shapes, cols = cfg.obs_layout(tag == "mgdm_shipped")
        assert [[k, v["use_normalizer"], list(v["shape"])] for k, v in shapes.items()] == table["obs_shapes"], tag
        width = sum(int(np.prod(r[2])) for r in table["obs_shapes"])
        assert width == table["obs_dim"] and (cols is None) == (tag in ("default", "no_root_h_tracking", "task_product", "no_root_tracking", "no_root_tracking_at_all"))
        if cols is not None:
            assert len(cols) == width and max(cols) < cfg.obs_dim + 5
            virt = np.arange(cfg.obs_dim + 5)              # a numbered virtual row: [fused row | root_h, tx, ty, 0 | clock]
            row = virt[np.array(cols)]
            seg = dict(zip([r[0] for r in table["obs_shapes"]], np.split(row, np.cumsum([int(np.prod(r[2])) for r in table["obs_shapes"]])[:-1])))
            assert list(seg["hf"]) == list(range(871, 1312))
            if "target_xy" in seg:
                assert list(seg["target_xy"]) == [1313, 1314]
            if "replan_t" in seg:
                assert list(seg["replan_t"]) == [1316]
            if over.get("global_root_height_obs"):
                assert list(seg["char_obs"]) == [1312] + list(range(136))
    for name, tree in g["shipped_configs"].items():
        env = tree["env"]
        cfg = TrackerConfig(env, km, 441)
        mg = float(env["fraction_dm_envs"]) < 1.0
        shapes, cols = cfg.obs_layout(bool(env.get("enable_replan_timer_obs", False)) and mg)
        if "ig_parkour_env" in name:
            assert cfg.has_target_xy_obs and list(shapes) == ["char_obs", "tar_obs", "tar_contacts", "char_contacts", "hf", "target_xy", "replan_t"]
            assert len(cols) == 1315 == g["variants"]["mgdm_shipped"]["obs_dim"]
        else:
            assert cols is None and cfg.obs_dim == 1312
    # every switch of the env configuration is accepted (global_obs / track_root off are kernel flags since round 4)
    both = TrackerConfig(dict(default_env_config()["env"], global_obs=True, track_root=False), km, 441)
    assert both.struct.global_obs == 1 and both.struct.track_root == 0


def test_mjcf_parser_matches_reference_parse():
    from parc_amd.anim.kin_char_model import KinCharModel
    from parc_amd.assets import humanoid_spec
    z = golden("g2_char")
    km = KinCharModel("cpu")
    km.load_char_file(humanoid_spec.write_mjcf())
    assert km.get_body_names() == [str(n) for n in z["body_names"]]
    np.testing.assert_array_equal(km._parent_indices.numpy(), z["parent"])
    np.testing.assert_allclose(km._local_translation.numpy(), z["local_translation"], atol=0)
    np.testing.assert_allclose(km._local_rotation.numpy(), z["local_rotation"], atol=0)
    np.testing.assert_array_equal([j.joint_type.value for j in km._joints], z["joint_type"])
    np.testing.assert_array_equal([j.dof_idx for j in km._joints], z["dof_idx"])
    for j, jt in enumerate(km._joints):
        if jt.axis is not None:
            np.testing.assert_allclose(jt.axis.numpy(), z["joint_axis"][j], atol=0)
    np.testing.assert_allclose(km._lower_dof_limits.numpy(), z["lower"], rtol=1e-6)
    np.testing.assert_allclose(km._upper_dof_limits.numpy(), z["upper"], rtol=1e-6)
    assert km.get_dof_size() == 28 and km.get_num_joints() == 15
    s = km.c_struct()
    assert s.num_bodies == 15 and s.dof_size == 28 and s.max_depth == 4
    assert list(s.depth)[:15] == [0, 1, 2, 2, 3, 4, 2, 3, 4, 1, 2, 3, 1, 2, 3]


def test_ray_template_matches_reference():
    from parc_amd.util import geom_util
    z = golden("g4_rays")
    pts = geom_util.get_xy_points_cone(torch.zeros(2), 0.05, 2, 60, 3, 3, 0.26179938779)
    assert pts.shape == (441, 2)
    np.testing.assert_allclose(pts.numpy(), z["ray_xy_points"], atol=1e-7)


def test_tracker_config_observation_layout():
    from parc_amd.anim.kin_char_model import KinCharModel
    from parc_amd.assets import humanoid_spec
    from parc_amd.envs.ig_parkour.default_config import default_env_config
    from parc_amd.tracker_core import TrackerConfig
    km = KinCharModel("cpu")
    km.load_char_file(humanoid_spec.write_mjcf())
    cfg = TrackerConfig(default_env_config()["env"], km, 441)
    z = golden("g6_step")
    assert cfg.obs_dim == 1312 and cfg.char_obs_dim == 136 and cfg.tar_obs_dim == 105
    np.testing.assert_allclose(list(cfg.struct.reward_w), z["reward_w"], rtol=1e-6)
    np.testing.assert_allclose(list(cfg.struct.dof_err_w)[:28], z["dof_err_w"], atol=0)
    assert list(cfg.struct.key_body_ids)[:4] == list(z["key_body_ids"])
    np.testing.assert_allclose(list(cfg.struct.tar_dt), z["tar_obs_steps"].astype(np.float32) * np.float32(1 / 30.0), rtol=1e-6)
    # (until round 3 global_obs raised NotImplementedError; every switch of the env YAML is a kernel flag or a column layout since round 4)
    world = default_env_config()["env"]
    world["global_obs"] = True
    assert TrackerConfig(world, km, 441).struct.global_obs == 1 and cfg.struct.global_obs == 0


def test_safe_motion_reader_roundtrip(tmp_path):
    """The non-executing reader returns the same arrays pickle would, and refuses to run callables."""
    from parc_amd.util import safe_pickle
    from parc_amd.util.terrain_util import SubTerrain
    import parc_amd
    parc_amd.install_reference_aliases()
    ter = SubTerrain("terrain", 6, 5, 0.4, 0.4, -1.0, 2.0, device="cpu")
    ter.hf[:] = torch.arange(30, dtype=torch.float32).reshape(6, 5)
    data = {"fps": 30, "loop_mode": "CLAMP", "frames": np.random.rand(7, 34).astype(np.float32),
            "contacts": np.ones((7, 15), np.float32), "terrain": ter.numpy_copy()}
    p = tmp_path / "clip.pkl"
    with open(p, "wb") as f:
        pickle.dump(data, f)
    out = safe_pickle.load_motion_file_safe(str(p))
    np.testing.assert_array_equal(out["frames"], data["frames"])
    np.testing.assert_array_equal(out["terrain"]["hf"], ter.hf.numpy())
    assert out["terrain"]["__class__"].endswith("terrain_util.SubTerrain")
    np.testing.assert_allclose(out["terrain"]["min_point"], [-1.0, 2.0])

    class Evil:
        def __reduce__(self):
            return (os.system, ("echo pwned > /tmp/parc_pwned",))
    q = tmp_path / "evil.pkl"
    with open(q, "wb") as f:
        pickle.dump({"frames": Evil()}, f)
    out = safe_pickle.load_motion_file_safe(str(q))
    assert isinstance(out["frames"], safe_pickle.Unresolved)
    assert not os.path.exists("/tmp/parc_pwned")


def _dm_env_cpu(mode, tmp_path, n_clips=3, R=1):
    """DeepMimicEnv on CPU with synthetic clips + terrains (terrain tiling is host logic, no kernels)."""
    import types
    from parc_amd.envs.ig_parkour import dm_env
    from parc_amd.util import terrain_util
    rng = np.random.default_rng(3)
    ters = []
    for k in range(n_clips):
        nx, ny = 12 + 2 * k, 10 + k
        ters.append(terrain_util.SubTerrain.from_arrays(rng.integers(0, 3, (nx, ny)).astype(np.float32) * 0.3,
                                                         np.array([-1.0 - k, 0.5 * k], np.float32), np.array([0.4, 0.4], np.float32)))
    e = dm_env.DeepMimicEnv.__new__(dm_env.DeepMimicEnv)
    e._device = "cpu"
    e._terrain_build_mode = mode
    e._terrains_per_motion = R
    e._build_tile_meshes = True
    e._motion_lib = types.SimpleNamespace(_terrains=ters, num_motions=lambda: n_clips)
    return e, ters


def test_terrain_build_wide_places_every_clip_terrain(tmp_path):
    e, ters = _dm_env_cpu("wide", tmp_path, R=2)
    cfg = {"dm": {"heightmap": {"horizontal_scale": 0.4, "padding": 0.8}}}
    e.build_terrain(cfg, str(tmp_path / "t.pkl"))
    g = e._terrain
    assert e._dm_motion_offsets.shape == (3, 2, 2)
    for k, t in enumerate(ters):
        for j in range(2):
            # a clip-frame point + the offset lands on the same height in the global field
            p = t.min_point + e._dm_motion_offsets[k, j]
            ij = torch.round((p - g.min_point) / g.dxdy).long()
            sub = g.hf[ij[0]:ij[0] + t.hf.shape[0], ij[1]:ij[1] + t.hf.shape[1]]
            assert torch.equal(sub, t.hf)
    # the cache written next to it reloads through the non-executing reader
    e2, _ = _dm_env_cpu("wide", tmp_path)
    e2.load_terrain(str(tmp_path / "t.pkl"))
    assert torch.equal(e2._terrain.hf, g.hf) and torch.equal(e2._dm_motion_offsets, e._dm_motion_offsets)
    assert e2._terrains_per_motion == 2


def test_terrain_build_file_mode(tmp_path):
    import yaml
    from parc_amd.util import terrain_util
    e, ters = _dm_env_cpu("file", tmp_path, n_clips=2)
    big = terrain_util.SubTerrain.from_arrays(np.arange(80, dtype=np.float32).reshape(8, 10), np.array([-2.0, -3.0], np.float32),
                                              np.array([0.4, 0.4], np.float32))
    terrain_util.dump_reference_pickle({"terrain": big.numpy_copy()}, str(tmp_path / "ter.pkl"))
    for k, off in enumerate([None, np.array([1.2, -0.4], np.float32)]):
        d = {"fps": 30, "loop_mode": "CLAMP", "frames": np.zeros((4, 34), np.float32)}
        if off is not None:
            d["min_point_offset"] = off
        with open(tmp_path / "m{}.pkl".format(k), "wb") as f:
            pickle.dump(d, f)
    with open(tmp_path / "motions.yaml", "w") as f:
        yaml.safe_dump({"terrain": str(tmp_path / "ter.pkl"),
                        "motions": [{"file": str(tmp_path / "m0.pkl"), "weight": 1.0}, {"file": str(tmp_path / "m1.pkl"), "weight": 1.0}]}, f)
    e.build_terrain({"dm": {"motion_file": str(tmp_path / "motions.yaml")}}, None)
    assert e._terrains_per_motion == 1
    np.testing.assert_array_equal(e._terrain.hf.numpy(), big.hf.numpy())
    np.testing.assert_allclose(e._dm_motion_offsets.numpy(), np.array([[[0, 0]], [[1.2, -0.4]]], np.float32))
    # the shared terrain's voxel mesh is returned like the reference does (one entry, 4 verts per cell)
    assert len(e._all_terrain_verts) == 1 and e._all_terrain_verts[0][0].shape == (8 * 10 * 4, 3)
    assert e._all_terrain_tris[0][0].shape == (2 * 80 + 2 * 7 * 10 + 2 * 8 * 9, 3)


def test_voxel_mesh_matches_reference_and_shipped_arrays():
    """G10: the whole-array mesh builder against (A) the vertex / triangle arrays the reference's authors shipped in
    data/terrains/civilization_ig.pkl for the 50x50 civilization terrain and (B) the reference function run on a small
    field with a skirt: bit-exact, vertices and indices."""
    from parc_amd.util import terrain_util
    z = golden("g10_voxel_mesh")
    v, t = terrain_util.convert_heightfield_to_voxelized_trimesh(torch.tensor(z["a_hf"]), float(z["a_min_point"][0]), float(z["a_min_point"][1]),
                                                                 float(z["a_dx"]), padding=0)
    assert v.dtype == np.float32 and t.dtype == np.uint32 and v.shape == (10000, 3) and t.shape == (14800, 3)
    np.testing.assert_array_equal(v, z["a_verts"])
    np.testing.assert_array_equal(t, z["a_tris"])
    v, t = terrain_util.convert_heightfield_to_voxelized_trimesh(z["b_hf"], float(z["b_min_point"][0]), float(z["b_min_point"][1]),
                                                                 float(z["b_dx"]), padding=float(z["b_padding"]))
    np.testing.assert_array_equal(v, z["b_verts"])
    np.testing.assert_array_equal(t, z["b_tris"])
    # 1 x n and n x 1 fields have no edges along the collapsed axis
    v, t = terrain_util.convert_heightfield_to_voxelized_trimesh(np.zeros((1, 3), np.float32), 0.0, 0.0, 0.5)
    assert v.shape == (12, 3) and t.shape == (6 + 0 + 4, 3)


def test_create_dataset_yaml_matches_reference(tmp_path):
    """G11: class-balanced dataset YAML (PARC/util/create_dataset.py) on the tree of tests/golden/dataset_tree.py: same entries,
    same order, same weights as the reference produced (tests/golden/g11_dataset_yaml.json)."""
    import json
    import sys
    import yaml
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import dataset_tree
    from parc_amd.util import create_dataset, terrain_util
    with open(os.path.join(REPO, "tests", "golden", "g11_dataset_yaml.json")) as f:
        gold = json.load(f)

    def make_terrain(hf):
        return terrain_util.SubTerrain.from_arrays(hf, np.zeros(2, np.float32), np.array([0.4, 0.4], np.float32)).numpy_copy()
    folders = dataset_tree.build(str(tmp_path), make_terrain, dataset_tree.FILES + [dataset_tree.BAD_LOSS_FILE], dump=terrain_util.dump_reference_pickle)
    out = tmp_path / "out.yaml"
    create_dataset.create_dataset_yaml(folders, out, None, False, True, gold["cut_classes"], *gold["max_dim"])
    got = yaml.safe_load(out.read_text())["motions"]
    assert [os.path.relpath(m["file"], str(tmp_path)) for m in got] == [m["file"] for m in gold["motions"]]
    np.testing.assert_allclose([m["weight"] for m in got], [m["weight"] for m in gold["motions"]], rtol=1e-12)
    # every class ends up with the same total weight
    tot = {}
    for m in got:
        c = m["file"].split(os.sep)[-2] if "sub" not in m["file"] else "running"
        tot[c] = tot.get(c, 0.0) + m["weight"]
    assert max(tot.values()) - min(tot.values()) < 1e-9
    if not torch.cuda.is_available():
        # the preprocessing step pushes every clip through the FK kernels: without a GPU it must fail loudly, not fall back
        import pytest
        with pytest.raises((RuntimeError, AssertionError, OSError)):
            create_dataset.create_dataset_yaml(folders, out, None, True)


def test_procgen_terrains_match_reference_under_seeds():
    """G12: boxes / stairs / curvy paths / gap-vault course reproduce the reference's heightfields (and course mesh) bit for
    bit when the torch, random and numpy generators are seeded alike."""
    import random
    from parc_amd.util import terrain_util
    z = golden("g12_procgen")

    def seed(k):
        torch.manual_seed(k)
        random.seed(k)
        np.random.seed(k)

    def ter(nx, ny, dx, mx, my):
        return terrain_util.SubTerrain("t", nx, ny, dx, dx, mx, my, device="cpu")
    seed(12)
    hf = torch.zeros((16, 16), dtype=torch.float32)
    terrain_util.add_boxes_to_hf2(hf, box_max_height=3.0, box_min_height=-3.0, num_boxes=10, box_max_len=10, box_min_len=5)
    np.testing.assert_array_equal(hf.numpy(), z["boxes_hf"])
    assert len(np.unique(z["boxes_hf"])) > 3
    seed(13)
    t = ter(24, 20, 0.4, -1.0, 0.5)
    terrain_util.add_stairs_to_hf(t, num_stairs=2)
    np.testing.assert_array_equal(t.hf.numpy(), z["stairs_hf"])
    seed(14)
    t = ter(30, 28, 0.4, -2.0, -3.0)
    terrain_util.gen_paths_hf(t, num_paths=3)
    np.testing.assert_array_equal(t.hf.numpy(), z["paths_hf"])
    seed(15)
    t = ter(6, 400, 0.1, 0.0, 0.0).numpy_copy()
    t2, v, tr = terrain_util.random_linear_parkour_course(t, gap_width=11, gap_height=-1.0, vault_width=1, vault_height=1.0,
                                                          num_padding_cells=4)
    np.testing.assert_array_equal(np.asarray(t2.hf), z["course_hf"])
    assert set(np.unique(z["course_hf"]).tolist()) == {-1.0, 0.0, 1.0}
    np.testing.assert_array_equal(v, z["course_verts"])
    np.testing.assert_array_equal(tr, z["course_tris"])


def test_char_point_samples_match_reference():
    """G13: body sample points of the capsule / box geoms (util/geom_util.py:725-869), bit for bit; the sphere points come
    from trimesh in the reference and are only checked for their construction (parity unpinned)."""
    from parc_amd.anim import kin_char_model as kcm
    from parc_amd.util import geom_util
    g = golden("g13_terrain_geometry")
    m = kcm.KinCharModel("cpu")
    m.load_char_file(kcm.default_char_file())
    full = geom_util.get_char_point_samples(m)
    for b in range(m.get_num_joints()):
        m._geoms[b] = [x for x in m._geoms[b] if x._shape_type != kcm.GeomType.SPHERE]
    pts = geom_util.get_char_point_samples(m)
    assert [p.shape[0] for p in pts] == g["pts_count"].tolist()
    assert np.array_equal(torch.cat(pts).numpy(), g["pts"])
    assert np.array_equal(geom_util.get_box_point_surface_samples(torch.tensor([0.0885, 0.045, 0.0275]), "cpu", num_slices=3, dim_x=4, dim_y=5).numpy(),
                          g["box_pts"])
    assert np.array_equal(geom_util.get_capsule_point_surface_samples(0.31, 0.055, "cpu", num_cylinder_slices=5, num_circle_points=6).numpy(),
                          g["capsule_pts"])
    sph = geom_util.get_sphere_point_surface_samples(0.09, "cpu")
    assert sph.shape == (12, 3) and np.allclose(sph.norm(dim=-1).numpy(), 0.09, atol=1e-7)
    # 6 sphere geoms of 12 points; pelvis, head and the two hands have nothing else (their placeholder point goes away)
    assert sum(p.shape[0] for p in full) == sum(p.shape[0] for p in pts) - 4 + 12 * 6


def test_slice_terrain_around_motion_matches_reference():
    from parc_amd.util import terrain_util
    g, civ = golden("g13_terrain_geometry"), golden("g5_hf_civ")
    ter = terrain_util.SubTerrain.from_arrays(torch.tensor(g["civ_hf"]), torch.tensor(g["civ_min_point"]), torch.tensor(g["civ_dxdy"]))
    sl, lf = terrain_util.slice_terrain_around_motion(g["slice_frames_in"], ter, padding=1.0)
    assert list(sl.hf.shape) == g["slice_dims"].tolist()
    assert np.array_equal(sl.hf.numpy(), g["slice_hf"]) and np.allclose(sl.min_point.numpy(), g["slice_min_point"], atol=1e-6)
    assert np.allclose(lf, g["slice_frames_out"], atol=1e-6)


def test_kernarg_offsets_of_post_step_kernel_match_code_object():
    """track_post_kernel reads argument structs directly from the kernel-argument segment (kernarg_late); the offsets it derives
    from the struct sizes must be the ones the compiler laid the arguments out at (and the ctypes mirrors must have the C sizes)."""
    import shutil
    import sys
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        import pytest
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_kernarg_offsets as cko
    meta = [(o, s) for o, s, k in cko.metadata_offsets() if k == "by_value"][:5]
    assert meta == cko.expected_offsets()


# ---------------------------------------------------------------------------------------------------------------
# Files written for the reference's readers, and the module names the reference's scripts import
# ---------------------------------------------------------------------------------------------------------------
NUMPY_GLOBALS = {("numpy._core.multiarray", "_reconstruct"), ("numpy.core.multiarray", "_reconstruct"), ("numpy", "ndarray"),
                 ("numpy", "dtype"), ("numpy._core.multiarray", "scalar"), ("numpy.core.multiarray", "scalar")}
TORCH_GLOBALS = {("torch._utils", "_rebuild_tensor_v2"), ("torch.storage", "_load_from_bytes"), ("collections", "OrderedDict")}


def pickle_globals(path):
    """Every class / function a pickle file names (GLOBAL and STACK_GLOBAL), found by disassembly."""
    import pickletools
    out, strings = set(), []
    with open(path, "rb") as f:
        data = f.read()
    for op, arg, _ in pickletools.genops(data):
        if op.name == "GLOBAL":
            out.add(tuple(arg.split(" ")))
        elif op.name in ("SHORT_BINUNICODE", "BINUNICODE", "UNICODE"):
            strings.append(arg)
        elif op.name == "STACK_GLOBAL":
            out.add((strings[-2], strings[-1]))
        elif op.name in ("BINGET", "LONG_BINGET"):
            strings.append(None)          # a memoised string: resolved below through the inert loader instead
    if any(None in g for g in out):
        from parc_amd.util import safe_pickle
        out = set()

        def walk(r):
            if isinstance(r, safe_pickle.Global):
                out.add((r.module, r.name))
            elif isinstance(r, safe_pickle.Call):
                walk(r.func), walk(r.args), walk(r.state)
            elif isinstance(r, safe_pickle.Obj):
                walk(r.cls), walk(r.args), walk(r.state)
            elif isinstance(r, dict):
                for k, v in r.items():
                    walk(k), walk(v)
            elif isinstance(r, (list, tuple)):
                for v in r:
                    walk(v)
        walk(safe_pickle.load_inert(data))
    return out


_FAKE_REFERENCE_READER = r"""
import pickle, sys, types
# stands for the reference's own util/terrain_util.py in a process that has never heard of parc_amd
util = types.ModuleType("util"); util.__path__ = []
tu = types.ModuleType("util.terrain_util")
class SubTerrain:
    pass
SubTerrain.__module__ = "util.terrain_util"
tu.SubTerrain = SubTerrain
sys.modules["util"] = util; sys.modules["util.terrain_util"] = tu
with open(sys.argv[1], "rb") as f:
    d = pickle.load(f)
t = d["terrain"]
assert type(t) is SubTerrain, type(t)
assert not any(m.startswith("parc_amd") for m in sys.modules), "reading the file pulled parc_amd in"
print(type(t.hf).__module__, tuple(t.hf.shape), sorted(t.__dict__))
"""


def test_written_files_name_only_reference_classes(tmp_path):
    """A recorded clip / terrain cache must unpickle in the REFERENCE (anim/motion_lib.py:240, dm_env.py:493-507): the only
    non-numpy / non-torch class a file may name is util.terrain_util.SubTerrain, and a plain pickle.load in a process
    without parc_amd must rebuild it."""
    import subprocess
    import sys
    from parc_amd.util import terrain_util
    assert terrain_util.SubTerrain.__module__ == "util.terrain_util"
    ter = terrain_util.SubTerrain("terrain", 6, 5, 0.4, 0.4, -1.0, 2.0, device="cpu")
    clip = {"fps": 30, "loop_mode": "CLAMP", "frames": np.zeros((7, 34), np.float32), "contacts": np.ones((7, 15), np.float32),
            "terrain": ter.numpy_copy()}
    p = str(tmp_path / "clip.pkl")
    terrain_util.dump_reference_pickle(clip, p)
    g = pickle_globals(p)
    assert ("util.terrain_util", "SubTerrain") in g and g - NUMPY_GLOBALS == {("util.terrain_util", "SubTerrain")}, g
    out = subprocess.run([sys.executable, "-c", _FAKE_REFERENCE_READER, p], capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[0] == "numpy" and "(6, 5)" in out.stdout
    # the terrain cache of the `square` / `wide` build modes: torch tensors inside, like the reference's (dm_env.py:344-354)
    e, _ = _dm_env_cpu("wide", tmp_path, R=2)
    cache = str(tmp_path / "terrain.pkl")
    e.build_terrain({"dm": {"heightmap": {"horizontal_scale": 0.4, "padding": 0.8}}}, cache)
    g = pickle_globals(cache)
    assert g - NUMPY_GLOBALS - TORCH_GLOBALS == {("util.terrain_util", "SubTerrain")}, g
    out = subprocess.run([sys.executable, "-c", _FAKE_REFERENCE_READER, cache], capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[0] == "torch"            # reference load_terrain calls .set_device / .to on these
    # ... and it also works while a foreign util.terrain_util is registered in THIS process (the writer swaps it in)
    import sys as _sys
    import types
    prev = _sys.modules.get("util.terrain_util")
    _sys.modules["util.terrain_util"] = types.ModuleType("util.terrain_util")
    try:
        terrain_util.dump_reference_pickle(clip, p)
        assert _sys.modules["util.terrain_util"] is not _sys.modules["parc_amd.util.terrain_util"]
    finally:
        _sys.modules["util.terrain_util"] = prev
    assert ("util.terrain_util", "SubTerrain") in pickle_globals(p)


def test_reference_module_names_resolve_strictly():
    """What run.py:7-12, parc_3_tracker.py:1-6 and parc_4_phys_record.py:1-6 import must resolve after
    install_reference_aliases(strict=True) in a fresh interpreter; a missing alias is an error, not a skip."""
    import subprocess
    import sys
    code = r"""
import parc_amd
parc_amd.install_reference_aliases(strict=True)
import envs.env_builder as env_builder
import learning.agent_builder as agent_builder
import util.arg_parser as arg_parser
from util.logger import Logger
import util.mp_util as mp_util
import util.util as util
from PARC.util.create_dataset import create_dataset_yaml_from_config
import util.torch_util as torch_util, util.terrain_util as terrain_util, util.geom_util, anim.kin_char_model, anim.motion_lib
import learning.base_agent as base_agent, learning.ppo_agent, learning.dm_ppo_agent, learning.experience_buffer
assert callable(env_builder.build_env) and callable(agent_builder.build_agent) and callable(create_dataset_yaml_from_config)
assert base_agent.AgentMode.TRAIN.value == 0 and hasattr(torch_util, "quat_rotate") and hasattr(terrain_util, "SubTerrain")
for name in parc_amd._ALIASES:
    __import__(name)
parc_amd._ALIASES["util.no_such_module"] = "util.no_such_module"
try:
    parc_amd.install_reference_aliases()
except ModuleNotFoundError:
    print("strict ok")
"""
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=REPO)
    assert out.returncode == 0 and "strict ok" in out.stdout, out.stderr


def test_g24_calls_of_the_reference_stage_scripts_resolve(tmp_path):
    """Fixture G24 = what the reference's OWN parc_3_tracker.train_tracker / parc_4_phys_record.record_motions emit and call when they
    run unchanged on this package's aliases (gen_golden.py stage stage-scripts, build container): the YAML files they write, the argv
    for run.main, every call run.run makes into the package (run.py:95-138).  Here: every recorded call binds to the signature this
    package offers under that name, with the argument kinds the reference passes; the written YAML parses into configs the builders
    accept key for key; the argv parses with this package's ArgParser into the same values.  (tests/test_dropin_gpu.py then feeds the
    very same files and argv to parc_amd.run.main on the GPU.)"""
    import inspect
    import yaml
    from parc_amd.envs import env_builder
    from parc_amd.envs.ig_parkour.default_config import default_agent_config, default_env_config
    from parc_amd.learning import agent_builder, dm_ppo_agent
    from parc_amd.util import arg_parser, mp_util, util as util_mod
    with open(os.path.join(REPO, "tests", "golden", "g24_stage_scripts.json")) as f:
        g = json.load(f)
    target = {"mp_util.init": mp_util.init, "util.set_rand_seed": util_mod.set_rand_seed, "env_builder.build_env": env_builder.build_env,
              "agent_builder.build_agent": agent_builder.build_agent, "agent.load": dm_ppo_agent.DMPPOAgent.load,
              "agent.train_model": dm_ppo_agent.DMPPOAgent.train_model, "agent.record_motions": dm_ppo_agent.DMPPOAgent.record_motions}
    want_calls = {"tracker_fresh": ["mp_util.init", "util.set_rand_seed", "env_builder.build_env", "agent_builder.build_agent", "agent.train_model"],
                  "tracker_resume": ["mp_util.init", "util.set_rand_seed", "env_builder.build_env", "agent_builder.build_agent", "agent.load", "agent.train_model"],
                  "record": ["mp_util.init", "util.set_rand_seed", "env_builder.build_env", "agent_builder.build_agent", "agent.load", "agent.record_motions"]}
    for name, run in g["runs"].items():
        assert [c["call"] for c in run["calls"]] == want_calls[name]
        for c in run["calls"]:
            fn = target[c["call"]]
            args = list(c["args"])
            if c["call"].startswith("agent."):
                args = ["<self>"] + args
            bound = inspect.signature(fn).bind(*args, **c["kwargs"])          # raises TypeError if the call does not fit
            if c["call"] == "env_builder.build_env":
                a = bound.arguments
                assert isinstance(a["num_envs"], int) and a["visualize"] is False and a["device"] == "cuda:0" and a["env_file"].endswith(".yaml")
            if c["call"] == "agent.train_model":
                assert set(c["kwargs"]) == {"max_samples", "out_model_file", "int_output_dir", "logger_type", "log_file"}
                assert c["kwargs"]["max_samples"] == 2048 and c["kwargs"]["logger_type"] == "tb"
            if c["call"] == "mp_util.init":
                assert c["args"][0:3] == [0, 1, "cuda:0"]
            if c["call"] == "util.set_rand_seed":
                util_mod.set_rand_seed(np.uint64(123456789012))                 # the reference hands over a numpy uint64 (run.py:82-93)
        # argv -> this package's ArgParser -> the same values the reference's parser handed to the calls
        assert len(run["argv"]) == 1
        ap = arg_parser.ArgParser()
        ap.load_args(run["argv"][0][1:])
        be = [c for c in run["calls"] if c["call"] == "env_builder.build_env"][0]["args"]
        assert [ap.parse_string("env_config"), ap.parse_int("num_envs", 1), ap.parse_string("device", "cuda:0"), ap.parse_bool("visualize", True)] == be
        assert ap.parse_string("mode", "train") == ("record" if name == "record" else "train")
    # the YAML the scripts wrote: the default trees with the three keys train_tracker patches (parc_3_tracker.py:30-36)
    env_y = yaml.safe_load(g["runs"]["tracker_resume"]["files_written_to_output_dir"]["dm_env.yaml"])
    ours = default_env_config()
    assert set(env_y) == set(ours) and set(env_y["env"]) == set(ours["env"]) and set(env_y["env"]["dm"]) == set(ours["env"]["dm"]) and env_y["sim"] == ours["sim"]
    assert env_y["env"]["dm"]["motion_file"] == "<TMP>/dataset/motions.yaml" and env_y["env"]["dm"]["terrain_save_path"] == "<TMP>/tracker_resume/terrain.pkl"
    ag_fresh = yaml.safe_load(g["runs"]["tracker_fresh"]["files_written_to_output_dir"]["agent_config.yaml"])
    ag_res = yaml.safe_load(g["runs"]["tracker_resume"]["files_written_to_output_dir"]["agent_config.yaml"])
    assert ag_fresh["normalizer_samples"] == 300000000 and ag_res["normalizer_samples"] == 0       # resuming freezes the normaliser
    assert set(ag_fresh) == set(default_agent_config())
    rec_y = yaml.safe_load(g["runs"]["record"]["files_written_to_output_dir"]["record_env.yaml"])
    assert rec_y["env"]["output_motion_dir"] == "<TMP>/record/recorded_motions" and rec_y["env"]["dm"]["terrain_save_path"] == "<TMP>/record/terrain.pkl"
    # record mode: one env per dataset entry (parc_4_phys_record.py:22-27); the dataset YAML came from this package's create_dataset
    n_motions = len(yaml.safe_load(g["dataset_yaml"])["motions"])
    assert [c for c in g["runs"]["record"]["calls"] if c["call"] == "env_builder.build_env"][0]["args"][1] == n_motions == 3


def test_importing_the_package_registers_no_top_level_names():
    """`import parc_amd...` must not redirect anybody's `import util` (round-2 advisor finding): nothing named util / envs / learning /
    anim appears in sys.modules until install_reference_aliases() is called; writing a reference-format file still works without it
    (dump_reference_pickle registers the path for the duration of the dump only), a plain pickle.dump of a SubTerrain does not."""
    import subprocess
    import sys
    code = r"""
import pickle, sys, io
import parc_amd, parc_amd.util.terrain_util as tu, parc_amd.envs.env_builder, parc_amd.learning.agent_builder, parc_amd.anim.motion_lib
import parc_amd.tools.motion_opt.motion_optimization, parc_amd.zmotion_editing_tools.motion_edit_lib
bad = [m for m in sys.modules if m.split(".")[0] in ("util", "envs", "learning", "anim", "PARC", "tools", "zmotion_editing_tools")]
assert bad == [], bad
t = tu.SubTerrain("terrain", 3, 3, 0.4, 0.4, 0.0, 0.0, device="cpu").numpy_copy()
try:
    pickle.dumps({"terrain": t})
    raise SystemExit("plain dump should not resolve util.terrain_util here")
except pickle.PicklingError:
    pass
tu.dump_reference_pickle({"terrain": t}, sys.argv[1])
assert [m for m in sys.modules if m.split(".")[0] == "util"] == []
parc_amd.install_reference_aliases()
import util.terrain_util
assert util.terrain_util is tu and pickle.loads(pickle.dumps({"terrain": t}))["terrain"].hf.shape == (3, 3)
print("ok")
"""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run([sys.executable, "-c", code, os.path.join(d, "t.pkl")], capture_output=True, text=True, cwd=REPO)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr


def test_g25_experience_buffer_table_and_sampler_walk(monkeypatch):
    """Fixture G25 (the reference's DMPPOAgent._build_exp_buffer chain and ExperienceBuffer on CPU, learning/experience_buffer.py:3-115,
    base_agent.py:224-253, ppo_agent.py:62-80, dm_ppo_agent.py:281-313): (1) this package's agent builds the same buffers - names in the
    same order, dtypes, shapes - plus exactly two named update-phase caches; (2) the sampler replays the reference's index walk call
    by call from the recorded torch.randperm draws: partly filled buffer (indices folded by the valid sample count), full buffer,
    calls that wrap in mid-call, a call for the whole buffer."""
    from parc_amd.learning import dm_ppo_agent, experience_buffer
    with open(os.path.join(REPO, "tests", "golden", "g25_experience_buffer.json")) as f:
        g = json.load(f)
    T_, N_ = g["T"], g["N"]

    class Space:
        def __init__(self, n):
            self.shape, self.dtype = (n,), np.float32

    class Env:
        NAME = "ig_parkour"

        def get_obs_space(self):
            return Space(1312)

        def get_action_space(self):
            return Space(28)

        def get_num_envs(self):
            return N_

    class Agent:
        _device, _steps_per_iter, _is_terrain_runner, _env = "cpu", T_, True, Env()

        def get_num_envs(self):
            return N_
    ag = Agent()
    dm_ppo_agent.DMPPOAgent._build_exp_buffer(ag, {})
    ours = [[k, str(v.dtype).replace("torch.", ""), list(v.shape)] for k, v in ag._exp_buffer._buffers.items()]
    extra = [b for b in ours if b[0] not in {r[0] for r in g["buffers"]}]
    assert [b for b in ours if b not in extra] == sorted(g["buffers"], key=lambda r: [o[0] for o in ours].index(r[0]))
    assert {b[0] for b in ours} - {b[0] for b in extra} == {r[0] for r in g["buffers"]}
    for r in g["buffers"]:
        assert r in ours, r                                                             # same name, dtype and shape
    assert [b[0] for b in extra] == ["norm_obs", "loss_rec"] and extra[0][2] == [T_, N_, 1312] and extra[1][2] == [T_, N_, 32]
    assert [[k, list(v.shape)] for k, v in ag._exp_buffer._flat_buffers.items() if k not in ("norm_obs", "loss_rec")] == \
        sorted(g["flat_views"], key=lambda r: [o[0] for o in ours].index(r[0]))
    # reference insertion order for the names both have, except that the two replan buffers come last here as there
    ref_names = [r[0] for r in g["buffers"]]
    assert [b[0] for b in ours if b[0] in ref_names] == ref_names
    # ---- sampler
    draws = [torch.tensor(p_, dtype=torch.long) for p_ in g["randperm_draws"]]
    it = iter(draws)
    monkeypatch.setattr(experience_buffer.torch, "randperm", lambda n, **k: next(it).clone())
    buf = experience_buffer.ExperienceBuffer(buffer_length=T_, batch_size=N_, device="cpu")
    # (the reference's constructor draws twice - allocation and _reset_sample_buf - this one once: skip the unused first draw)
    buf._reset_sample_buf()
    buf.add_buffer("x", torch.zeros([T_, N_, 2]))
    walk = iter(g["index_walk"])
    for t_ in range(2):
        buf.record("x", torch.full([N_, 2], float(t_ + 1)))
        buf.inc()
    for _ in range(2):
        w = next(walk)
        assert w["phase"] == "partly filled" and buf.get_sample_count() == w["sample_count"]
        assert buf._sample_rand_idx(w["n"]).tolist() == w["idx"] and buf._sample_buf_head == w["head_after"]
    for t_ in range(2, 7):
        buf.record("x", torch.full([N_, 2], float(t_ + 1)))
        buf.inc()
    assert buf._buffer_head == g["buffer_head_after_7_incs"] and buf.get_total_samples() == g["total_samples_after_7_incs"]
    assert buf.get_data("x")[:, 0, 0].tolist() == g["rows_after_7_records"]
    buf.reset()
    for w in walk:
        assert buf.get_sample_count() == w["sample_count"]
        got = buf._sample_rand_idx(w["n"])
        assert got.tolist() == w["idx"] and buf._sample_buf_head == w["head_after"], w
    assert list(buf.sample(4).keys()) == g["sample_keys"] and list(buf.sample(4, keys=["x"]).keys()) == ["x"]
    assert next(it, None) is None                                                       # every recorded draw was consumed, in order


def test_library_is_built_from_the_sources_beside_it():
    """lib() refuses a stale libparc_hip.so (argument structs of another layout would be handed to it): the digest build() stored
    equals the digest of csrc/ + include/ now, and a changed source is noticed."""
    from parc_amd import _hip
    assert _hip._stored_digest() == _hip.source_digest()
    old = _hip.OPT_LEVEL.get("parc_terrain.hip")
    _hip.OPT_LEVEL["parc_terrain.hip"] = "-O1"
    try:
        assert _hip._stored_digest() != _hip.source_digest()
    finally:
        if old is None:
            del _hip.OPT_LEVEL["parc_terrain.hip"]
        else:
            _hip.OPT_LEVEL["parc_terrain.hip"] = old


def test_every_source_is_built_with_its_flags():
    """A .hip file left out of the build, or one of the files measured without the SLP vectoriser silently built at the default -O3,
    would change the product without any other test failing."""
    import os
    from parc_amd import _hip
    on_disk = {f for f in os.listdir(_hip.CSRC) if f.endswith(".hip")}
    assert on_disk == set(_hip.DIAG_SOURCES) and len(_hip.DIAG_SOURCES) == len(on_disk)
    assert set(_hip.SOURCES) == set(_hip.DIAG_SOURCES) - {"parc_sim_ref.hip"} and len(_hip.SOURCES) == len(_hip.DIAG_SOURCES) - 1
    for f in ("parc_kin.hip", "parc_hfgather.hip", "parc_motion.hip", "parc_pose_opt.hip", "parc_returns.hip", "parc_sim.hip"):
        assert "-fno-slp-vectorize" in _hip.OPT_LEVEL[f].split(), f
    # the learner files were measured as one file at the default level and stay there
    for f in ("parc_ppo.hip", "parc_rollout.hip", "parc_optim.hip", "parc_colreduce.hip"):
        assert f in _hip.SOURCES and _hip.OPT_LEVEL.get(f, "-O3") == "-O3", f


def test_torch_util_matches_reference_fixture():
    """parc_amd/util/torch_util.py (served as util.torch_util) against fixture G1 (reference util/torch_util.py on CPU)."""
    from parc_amd.util import torch_util as tu
    z = golden("g1_quat")
    t = lambda k: torch.tensor(z[k])
    chk = lambda got, k, tol=2e-6: np.testing.assert_allclose(got.numpy(), z[k], atol=tol, rtol=0)
    chk(tu.quat_mul(t("a"), t("b")), "quat_mul")
    chk(tu.quat_rotate(t("a"), t("v")), "quat_rotate")
    chk(tu.exp_map_to_quat(t("exp_map")), "exp_map_to_quat")
    chk(tu.quat_to_exp_map(t("a")), "quat_to_exp_map", 1e-5)
    chk(tu.axis_angle_to_quat(t("axis"), t("angle")), "axis_angle_to_quat")
    chk(tu.quat_to_tan_norm(t("a")), "quat_to_tan_norm")
    chk(tu.slerp(t("a"), t("b"), t("blend")), "slerp", 1e-5)
    chk(tu.calc_heading(t("a")), "calc_heading", 1e-5)
    chk(tu.calc_heading_quat_inv(t("a")), "calc_heading_quat_inv", 1e-5)
    chk(tu.quat_diff_angle(t("a"), t("b")), "quat_diff_angle", 2e-5)


# ---------------------------------------------------------------------------------------------------------------
# Learner-side host classes against fixtures produced by the reference's own classes (G15, G16) and the reference's readers
# on files this package wrote (G19).  The device kernels are checked against the same fixtures in tests/test_learner_gpu.py.
# ---------------------------------------------------------------------------------------------------------------
def check_normalizer_against_g15(device):
    from parc_amd.learning.normalizer import Normalizer
    z = golden("g15_normalizer")
    T = lambda a, dt=torch.float32: torch.tensor(np.asarray(a), dtype=dt, device=device)
    nz = Normalizer((1312,), device, clip=float(z["clip"]), non_norm_indices=T(z["non_norm_indices"], torch.int64))
    for r in range(3):
        for k in range(2):
            nz.record(T(z["x_%d_%d" % (r, k)]))
            if r == 0 and k == 1:
                assert nz._new_count == int(z["new_count_r0"])
                np.testing.assert_allclose(nz._new_sum.cpu().numpy(), z["new_sum_r0"], rtol=2e-6, atol=2e-4)
                np.testing.assert_allclose(nz._new_sum_sq.cpu().numpy(), z["new_sum_sq_r0"], rtol=2e-6, atol=2e-3)
        nz.update()
        assert int(nz._count.item()) == int(z["count_%d" % r][0])
        np.testing.assert_allclose(nz._mean.cpu().numpy(), z["mean_%d" % r], rtol=1e-5, atol=2e-6)
        std, ref_std = nz._std.cpu().numpy().copy(), z["std_%d" % r].copy()
        if r == 0:                               # column 5 is constant in round 0: its variance is fp32 cancellation noise, which
            assert std[5] < 2e-3 and ref_std[5] < 2e-3      # depends on the summation order; everything else must agree
            std[5] = ref_std[5] = 0.0
        # std = sqrt(E[x^2] - E[x]^2) in fp32 (normalizer.py:88-93): a column whose spread is small against its mean loses digits
        # to cancellation, by an amount that depends on the summation order -> tolerance from the conditioning of that formula
        ref_mean = z["mean_%d" % r]
        tol = 2e-4 * ref_std + 2e-6 + 8 * 1.2e-7 * (ref_mean ** 2 + ref_std ** 2) / np.maximum(ref_std, 1e-4)
        assert np.all(np.abs(std - ref_std) <= tol), np.nonzero(np.abs(std - ref_std) > tol)
        assert np.mean(np.abs(std - ref_std) <= 2e-4 * ref_std + 2e-6) > 0.99
    assert torch.all(nz._mean[766:] == 0) and torch.all(nz._std[766:] == 1)
    # normalise with the REFERENCE's statistics, so that the comparison is about normalize() alone
    nz._mean[:] = T(z["mean_2"])
    nz._std[:] = T(z["std_2"])
    q = T(z["query"])
    np.testing.assert_allclose(nz.normalize(q).cpu().numpy(), z["normalized"], rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(nz.unnormalize(q).cpu().numpy(), z["unnormalized"], rtol=2e-6, atol=2e-6)
    an = Normalizer((28,), device, init_mean=T(0.5 * (z["a_high"] + z["a_low"])), init_std=T(0.5 * (z["a_high"] - z["a_low"])))
    np.testing.assert_array_equal(an._mean.cpu().numpy(), z["a_mean"])
    np.testing.assert_array_equal(an._std.cpu().numpy(), z["a_std"])
    np.testing.assert_allclose(an.unnormalize(T(z["norm_action"])).cpu().numpy(), z["action"], rtol=1e-6, atol=1e-6)


def check_trackers_against_g16(device):
    from parc_amd.learning.dm_ppo_return_tracker import DMPPOReturnTracker
    from parc_amd.learning.tracking_error_tracker import TrackingErrorTracker
    z = golden("g16_trackers")
    keys = [str(k) for k in z["keys"]]
    S, K, N = z["rewards"].shape
    tr, te = DMPPOReturnTracker(N, device), TrackingErrorTracker(N, device)
    T = lambda a, dt=torch.float32: torch.tensor(np.asarray(a), dtype=dt, device=device)
    for s in range(S):
        block = T(z["rewards"][s])
        info = {"rewards": {k: block[i] for i, k in enumerate(keys)}, "rewards_all": (keys, block)}
        done = T(z["done"][s], torch.int32)
        tr.update(info, done)
        te.update(T(z["tracking_error"][s]), done)
        got = np.array([tr.get_specific_mean_return(k).item() for k in keys], np.float32)
        np.testing.assert_allclose(got, z["mean_returns"][s], rtol=3e-6, atol=1e-6, err_msg="step %d" % s)
        assert tr.get_mean_ep_len().item() == pytest.approx(float(z["mean_ep_len"][s]), rel=3e-6)
        assert tr.get_episodes() == int(z["episodes"][s])
        np.testing.assert_allclose(te._mean.cpu().numpy(), z["te_means"][s], rtol=3e-6, atol=1e-6, err_msg="step %d" % s)
    np.testing.assert_array_equal(tr.get_eps_per_env().cpu().numpy(), z["eps_per_env"])
    np.testing.assert_allclose(tr._return_buf.cpu().numpy(), z["return_bufs"], rtol=1e-6, atol=1e-6)
    np.testing.assert_array_equal(tr._ep_len_buf.cpu().numpy(), z["ep_len_buf"])
    assert tr.get_mean_return().item() == pytest.approx(float(z["mean_returns"][-1, 0]), rel=3e-6)


def test_g15_normalizer_host_path():
    check_normalizer_against_g15("cpu")


def test_g16_trackers_host_path():
    check_trackers_against_g16("cpu")


def test_g19_reference_read_our_recorded_files():
    """tests/golden/recorded/ holds a clip written by record mode and a terrain cache written by the env, both on the GPU
    (tools/make_recorded_fixture.py).  gen_golden.py opened them with the reference's MotionLib / load_terrain and stored what it
    read (G19); here the same files, read by this package, must hold the same data - and name only reference classes."""
    from parc_amd.util import safe_pickle
    z = golden("g19_recorded_files")
    rec_dir = os.path.join(REPO, "tests", "golden", "recorded")
    clip = os.path.join(rec_dir, "recorded_clip_dm.pkl")
    sub = {("util.terrain_util", "SubTerrain")}
    assert pickle_globals(clip) - NUMPY_GLOBALS - {("collections", "OrderedDict")} == sub
    assert pickle_globals(os.path.join(rec_dir, "terrain.pkl")) - NUMPY_GLOBALS - TORCH_GLOBALS == sub
    d = safe_pickle.load_motion_file_safe(clip)
    F = int(z["num_frames"][0])
    assert d["frames"].shape == (F, 34) and d["fps"] == int(z["fps"][0]) and d["loop_mode"] == "CLAMP" and int(z["loop_mode"][0]) == 0
    np.testing.assert_array_equal(d["frames"][:, 0:3], z["frame_root_pos"])
    np.testing.assert_array_equal(d["contacts"], z["frame_contacts"])
    np.testing.assert_array_equal(d["obs"], z["obs"])
    assert list(d["obs_shapes"].keys()) == [str(k) for k in z["obs_shape_names"]]
    t = d["terrain"]
    np.testing.assert_array_equal(t["hf"], z["ter_hf"])
    np.testing.assert_array_equal(np.asarray(t["min_point"]), z["ter_min_point"])
    np.testing.assert_array_equal(np.asarray(t["dxdy"]), z["ter_dxdy"])
    np.testing.assert_array_equal(np.asarray(t["dims"]), z["ter_dims"])
    np.testing.assert_array_equal(np.asarray(t["hf_mask"]), z["ter_hf_mask"])
    # the terrain cache through this package's own load_terrain
    e, _ = _dm_env_cpu("square", None)
    verts, tris = e.load_terrain(os.path.join(rec_dir, "terrain.pkl"))
    np.testing.assert_array_equal(e._terrain.hf.numpy(), z["cache_hf"])
    np.testing.assert_array_equal(e._terrain.min_point.numpy(), z["cache_min_point"])
    np.testing.assert_array_equal(e._dm_motion_offsets.numpy(), z["cache_motion_offsets"])
    assert e._terrains_per_motion == int(z["cache_terrains_per_motion"]) and len(verts) == int(z["cache_num_vert_lists"])
    np.testing.assert_array_equal(np.asarray(verts[0][0]), z["cache_verts_0"])
    np.testing.assert_array_equal(np.asarray(tris[0][0]), z["cache_tris_0"])


def test_optimiser_output_file_is_reference_readable():
    """What tools/motion_opt/optimize_motions.py:182-193 writes - a motion dict whose "opt:body_constraints" holds BodyConstraint
    objects - names only the reference's module paths, and the run-splitting rule of the constraint builder (a trailing one-frame
    run is dropped, extract_consecutive_trues :43-73) is the reference's."""
    import pickle
    import tempfile
    import parc_amd
    from parc_amd.tools.motion_opt import motion_optimization as mo
    from parc_amd.util import terrain_util
    runs = mo._consecutive_true_runs(torch.tensor([0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 1], dtype=torch.bool))
    assert [r.tolist() for r in runs] == [[1, 2], [4], [7, 8, 9]]
    assert mo._consecutive_true_runs(torch.tensor([0, 0, 1, 0], dtype=torch.bool)) == []          # the reference's rule, as is
    assert [r.tolist() for r in mo._consecutive_true_runs(torch.tensor([1, 1, 1], dtype=torch.bool))] == [[0, 1, 2]]
    ter = terrain_util.SubTerrain.from_arrays(np.zeros((4, 5), np.float32), np.zeros(2, np.float32), np.array([0.4, 0.4], np.float32), device="cpu")
    c = mo.BodyConstraint()
    c.start_frame_idx, c.end_frame_idx, c.constraint_point = 3, 9, torch.tensor([0.1, 0.2, 0.3])
    data = {"fps": 30, "loop_mode": "CLAMP", "frames": torch.zeros((12, 34)), "contacts": torch.zeros((12, 15)), "terrain": ter,
            "opt:body_constraints": [[c], []]}
    path = os.path.join(tempfile.mkdtemp(prefix="parc_opt_"), "clip_opt.pkl")
    terrain_util.dump_reference_pickle(data, path)
    mods = {m for m, _ in pickle_globals(path)}
    assert ("tools.motion_opt.motion_optimization", "BodyConstraint") in pickle_globals(path)
    assert not any(m.startswith("parc_amd") for m in mods), mods
    parc_amd.install_reference_aliases()
    back = pickle.load(open(path, "rb"))                               # a file of our own
    assert back["opt:body_constraints"][0][0].end_frame_idx == 9


def test_mgdm_terrain_build_and_pose_containers_against_g21(tmp_path):
    """Host side of the motion-generator sub-env against fixture G21 (the reference's mgdm_env.py on CPU): the checkerboard platform
    terrain with the same Python RNG stream, its spawn bounds and voxel-mesh size, the generator's local grid, the cache file's class
    paths; MotionFrames container operations."""
    import json
    import random
    import parc_amd
    from parc_amd.anim.kin_char_model import KinCharModel
    from parc_amd.assets import humanoid_spec
    from parc_amd.envs.ig_parkour import mgdm_env
    from parc_amd.util import motion_util
    g = golden("g21_mgdm")
    km = KinCharModel("cpu")
    km.load_char_file(humanoid_spec.write_mjcf())

    class Gen:
        _num_prev_states, _sequence_fps = 2, 30
        _dx = _dy = 0.4
        _num_x_neg, _num_x_pos, _num_y_neg, _num_y_pos = 2, 5, 3, 3
    cfg = json.loads(bytes(g["config_json"]).decode())
    env = mgdm_env.MotionGenDeepMimicEnv(cfg, 8, "cpu", False, km, generator=Gen())
    np.testing.assert_allclose(env._mgdm_local_xy_points.numpy(), g["local_grid"], atol=1e-6)
    random.seed(21)
    path = str(tmp_path / "mgdm_terrain.pkl")
    verts, tris, min_point = env.build_terrain(cfg["env"], path)
    np.testing.assert_array_equal(env._terrain.hf.numpy(), g["terrain_hf"])
    np.testing.assert_allclose(env._terrain.min_point.numpy(), g["terrain_min_point"], atol=0)
    np.testing.assert_allclose([env._spawn_min_x, env._spawn_max_x, env._spawn_min_y, env._spawn_max_y, env._oob_region], g["spawn"], atol=1e-12)
    assert [verts.shape[0], tris.shape[0]] == g["mesh_counts"].tolist()
    assert {m for m, _ in pickle_globals(path) if not m.startswith(("numpy", "torch", "collections", "_codecs"))} == {"util.terrain_util"}
    env2 = mgdm_env.MotionGenDeepMimicEnv(cfg, 8, "cpu", False, km, generator=Gen())
    env2.load_terrain(path)
    assert torch.equal(env2._terrain.hf, env._terrain.hf) and env2._spawn_max_x == env._spawn_max_x and env2._oob_region == env._oob_region
    assert env.get_target_dim() == 2
    # the package opens no model file and imports nothing of the reference's diffusion package (its load_mdm, mgdm_env.py:32-35, unpickles
    # a model object): without a generator callable the sub-env refuses, and mgdm.model_path points the user at INTEGRATION.md
    cfg_model = json.loads(bytes(g["config_json"]).decode())
    assert cfg_model["env"]["mgdm"]["model_path"]
    with pytest.raises(RuntimeError, match="mgdm.generator.*INTEGRATION.md"):
        mgdm_env.MotionGenDeepMimicEnv(cfg_model, 8, "cpu", False, km)
    cfg_model["env"]["mgdm"]["unsafe_pickle"] = True                 # the round-2 opt-in switch no longer exists
    with pytest.raises(RuntimeError, match="mgdm.generator"):
        mgdm_env.MotionGenDeepMimicEnv(cfg_model, 8, "cpu", False, km)
    del cfg_model["env"]["mgdm"]["model_path"]
    with pytest.raises(RuntimeError, match="need a planner"):
        mgdm_env.MotionGenDeepMimicEnv(cfg_model, 8, "cpu", False, km)
    assert not hasattr(mgdm_env, "ReferenceMDMGenerator")
    # pose containers
    a = motion_util.MotionFrames()
    a.init_blank_frames(km, 2, batch_size=3)
    assert a.joint_rot.shape == (3, 2, 14, 4) and float(a.root_rot[..., 3].min()) == 1.0
    b = motion_util.MotionFrames(root_pos=torch.ones(3, 1, 3), root_rot=a.root_rot[:, :1], joint_rot=a.joint_rot[:, :1], contacts=torch.zeros(3, 1, 15))
    a.body_pos = a.body_rot = None
    c = motion_util.cat_motion_frames([a, b])
    assert c.root_pos.shape == (3, 3, 3) and c.body_pos is None and float(c.root_pos[:, -1].min()) == 1.0
    assert c.get_slice(slice(1, 3)).contacts.shape == (3, 2, 15) and c.get_idx(torch.tensor([2])).root_pos.shape == (1, 3, 3)
    a.set_vals(c.get_slice(slice(1, 3)), torch.tensor([1]))
    assert float(a.root_pos[1, -1].min()) == 1.0 and float(a.root_pos[0].abs().max()) == 0.0
    parc_amd.install_reference_aliases()
    import util.motion_util as ref_named            # the name the reference's scripts import
    assert ref_named.MotionFrames is motion_util.MotionFrames


def test_motion_file_helpers_against_g22(tmp_path):
    """zmotion_editing_tools.motion_edit_lib on the host, against the reference's outputs (fixture G22): the mirrored terrain, and a
    motion file written by save_motion_data / MotionData.save_to_file - class paths, round trip through the non-executing reader."""
    import parc_amd
    from parc_amd.util import terrain_util
    from parc_amd.zmotion_editing_tools import motion_edit_lib as medit
    g = golden("g22_motion_edit")
    ter = terrain_util.SubTerrain.from_arrays(g["ter_hf"], g["ter_min_point"], g["ter_dxdy"], g["ter_mask"], g["ter_maxmin"], device="cpu")
    ter.flip_by_XZ_axis()
    np.testing.assert_array_equal(ter.hf.numpy(), g["ter_flip_hf"])
    np.testing.assert_array_equal(ter.hf_mask.numpy(), g["ter_flip_mask"])
    np.testing.assert_array_equal(ter.hf_maxmin.numpy(), g["ter_flip_maxmin"])
    np.testing.assert_allclose(ter.min_point.numpy(), g["ter_flip_min_point"], atol=1e-6)
    path = str(tmp_path / "clip.pkl")
    ter2 = terrain_util.SubTerrain.from_arrays(g["rt_hf"], np.zeros(2, np.float32), np.array([0.4, 0.4], np.float32), device="cpu")
    medit.save_motion_data(path, torch.tensor(g["frames"]), torch.tensor(g["contacts"]), ter2, 30, "CLAMP", loss=1.5,
                           min_point_offset=torch.tensor([0.25, -0.5]))
    mods = {m for m, _ in pickle_globals(path)}
    assert ("util.terrain_util", "SubTerrain") in pickle_globals(path) and not any(m.startswith("parc_amd") for m in mods), mods
    md = medit.load_motion_file(path)
    assert sorted(md._data.keys()) == [str(k) for k in g["rt_keys"]]
    assert md.get_fps() == int(g["rt_fps"][0]) and md.get_loop_mode() == "CLAMP" and md.has_terrain() and md.has_contacts()
    np.testing.assert_array_equal(md.get_frames().numpy(), g["rt_frames"])
    np.testing.assert_array_equal(md.get_contacts().numpy(), g["rt_contacts"])
    np.testing.assert_array_equal(md.get_terrain().hf.numpy(), g["rt_hf"])
    md.set_fps(29.97)
    path2 = str(tmp_path / "clip2.pkl")
    md.save_to_file(path2, verbose=False)
    back = medit.load_motion_file(path2)
    assert back.get_fps() == 29 and torch.equal(back.get_frames(), torch.tensor(g["rt_frames"]))      # int() of the value, like the reference
    parc_amd.install_reference_aliases()
    import zmotion_editing_tools.motion_edit_lib as by_reference_name
    assert by_reference_name.MotionData is medit.MotionData


def test_unsafe_pickle_opt_in_resolves_the_reference_class_paths_without_aliases(tmp_path):
    """safe_pickle.load_executing - the explicit `unsafe_pickle` opt-in of MotionLib / DeepMimicEnv / motion_edit_lib for files the user
    wrote - on a file that embeds a SubTerrain: the pickle names the class `util.terrain_util.SubTerrain` (the reference's path, what
    dump_reference_pickle writes); the load resolves it to this package although install_reference_aliases() was never called and
    importing the package registers nothing in sys.modules (round-3 advisor finding: ModuleNotFoundError: No module named 'util')."""
    import subprocess
    import sys
    code = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
from parc_amd.util import safe_pickle, terrain_util
assert "util" not in sys.modules and "util.terrain_util" not in sys.modules
ter = terrain_util.SubTerrain.from_arrays(np.arange(12, dtype=np.float32).reshape(3, 4), np.array([-1.0, 2.0], np.float32), np.array([0.4, 0.4], np.float32))
path = %r
terrain_util.dump_reference_pickle({"fps": 30, "loop_mode": "CLAMP", "frames": np.zeros((5, 34), np.float32), "terrain": ter}, path)
assert b"util.terrain_util" in open(path, "rb").read() and "util" not in sys.modules
d = safe_pickle.load_executing(path)
assert type(d["terrain"]) is terrain_util.SubTerrain and d["terrain"].hf.shape == (3, 4) and float(d["terrain"].hf[2, 3]) == 11.0
assert "util" not in sys.modules and "util.terrain_util" not in sys.modules          # nothing stays registered
from parc_amd.zmotion_editing_tools import motion_edit_lib
m = motion_edit_lib.load_motion_file(path, unsafe_pickle=True) if "unsafe_pickle" in motion_edit_lib.load_motion_file.__code__.co_varnames else None
print("ok")
""" % (REPO, str(tmp_path / "clip.pkl"))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "ok" in res.stdout, res.stderr[-3000:]
