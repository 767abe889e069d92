"""Host-side logic that needs no GPU: spaces, task descriptions, registry, sharding and the
world_size-2 gloo gather of rollout blocks."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


def test_task_descriptions_mirror_reference_defaults():
    from mujoco_sim_amd.environments.tasks.point_reach import (CONTROL_TIMESTEP, GOAL_DISTANCE_THRESHOLD, MAX_STEP_SIZE,
                                                               PHYSICS_TIMESTEP, PointMassReachTask)
    from mujoco_sim_amd.environments.tasks.robot_reach import RobotReachConfig, RobotReachTask

    t = PointMassReachTask()
    assert (t.reward_type, t.observation_type, t.image_resolution) == ("dense_biased_negative_distance_reward", "visual_observations", 64)
    assert (PHYSICS_TIMESTEP, CONTROL_TIMESTEP, GOAL_DISTANCE_THRESHOLD, MAX_STEP_SIZE) == (0.02, 0.1, 0.02, 0.05)
    spec = t.action_spec()
    assert spec.shape == (2,) and spec.dtype == np.float32 and np.allclose(spec.maximum, 0.05)
    with pytest.raises(AssertionError):
        PointMassReachTask(reward_type="nope")
    c = RobotReachConfig()
    assert (c.reward_type, c.observation_type, c.action_type) == ("dense_negative_distance_reward", "state_observations", "absolute_eef_action")
    assert (c.physics_timestep, c.control_timestep, c.max_control_steps_per_episode, c.goal_distance_threshold) == (0.005, 0.1, 100, 0.02)
    spec = RobotReachTask(c).action_spec()
    assert spec.dtype == np.float64 and np.allclose(spec.minimum, [-0.1, -0.6, 0.02]) and np.allclose(spec.maximum, [0.1, -0.4, 0.2])
    with pytest.raises(NotImplementedError):
        RobotReachTask(RobotReachConfig(action_type=RobotReachConfig.ABS_JOIN_ACTION))


def test_contact_task_descriptions_mirror_reference_defaults():
    from mujoco_sim_amd.environments.tasks.robot_planar_push import RobotPushConfig, RobotPushTask
    from mujoco_sim_amd.environments.tasks.robot_push_button import RobotPushButtonTask

    t = RobotPushButtonTask()  # robot_push_button.py:20-58
    assert (t.reward_type, t.observation_type, t.action_type, t.image_resolution) == ("sparse_reward", "visual_observations", "absolute_joint_action", 96)
    assert (t.PHYSICS_TIMESTEP, t.CONTROL_TIMESTEP, t.MAX_CONTROL_STEPS_PER_EPISODE, t.GOAL_DISTANCE_THRESHOLD) == (0.005, 0.1, 100, 0.05)
    assert t.use_wrist_camera and not t.button_disturbances and np.allclose(t.robot_end_position, [-0.3, -0.2, 0.3])
    spec = t.action_spec()
    assert spec.shape == (7,) and spec.dtype == np.float64 and np.allclose(spec.maximum, [3.14] * 6 + [0.085]) and np.allclose(spec.minimum, [-3.14] * 6 + [0.0])
    spec = RobotPushButtonTask(action_type="absolute_eef_action").action_spec()
    assert spec.shape == (4,) and np.allclose(spec.minimum, [-0.2, -0.6, 0.02, 0.0]) and np.allclose(spec.maximum, [0.2, -0.3, 0.3, 0.085])
    with pytest.raises(AssertionError):
        RobotPushButtonTask(action_type="relative_eef_action")
    c = RobotPushConfig()  # robot_planar_push.py:28-73
    assert (c.reward_type, c.observation_type) == ("dense_negative_distance_reward", "state_observations")
    assert (c.physics_timestep, c.control_timestep, c.max_control_steps_per_episode, c.target_radius, c.nearest_object_reward_coefficient) == (0.005, 0.1, 500, 0.05, 0.1)
    spec = RobotPushTask(c).action_spec()
    assert spec.shape == (2,) and spec.dtype == np.float32 and np.allclose(spec.maximum, 1.0)
    assert c.n_objects == 5  # robot_planar_push.py:61
    with pytest.raises(NotImplementedError):
        RobotPushConfig(n_objects=6)  # MJS_PP_MAX_OBJECTS = 5 block slots
    with pytest.raises(AssertionError):
        RobotPushConfig(reward_type="nope")


def test_spaces_and_registry():
    import mujoco_sim_amd as m
    from mujoco_sim_amd.environments.dmc2gym import _convert_specs_to_flattened_box, _flatten_obs, convert_spec_to_box
    from mujoco_sim_amd.environments.tasks.point_reach import ArraySpec, BoundedArraySpec

    assert "mujoco_sim/point_mass_reach-v0" in m.registry  # reference id (mujoco_sim/__init__.py:26-30)
    assert "mujoco_sim/robot_push_button_visual-v0" in m.registry  # reference id (mujoco_sim/__init__.py:31-39)
    box = _convert_specs_to_flattened_box([BoundedArraySpec((2,), np.float32, [-1, -2], [1, 2]), ArraySpec((2, 2), np.float64)], np.float64)
    assert box.shape == (6,) and box.dtype == np.float32 and np.isinf(box.high[2:]).all()
    b = convert_spec_to_box(BoundedArraySpec((3,), np.float64, -1, 1))
    assert b.dtype == np.float64 and b.shape == (3,)
    flat = _flatten_obs({"a": np.arange(2.0), "b": np.arange(6.0).reshape(2, 3)})
    assert flat.shape == (8,)
    with pytest.raises(KeyError):
        m.make("mujoco_sim/nope-v0")


def test_shard_range():
    from mujoco_sim_amd.distributed import shard_range

    assert [shard_range(4096, 8, r) for r in (0, 1, 7)] == [(0, 512), (512, 1024), (3584, 4096)]
    with pytest.raises(ValueError):
        shard_range(10, 4, 0)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, str(ROOT))
    import oracle
    from mujoco_sim_amd import distributed as D

    D.init_process_group("gloo")
    N, T = 8, 6
    lo, hi = D.shard_range(N, world, rank)
    # each rank steps ITS shard (oracle stands in for the GPU engine on this CPU-only test) with global seeds
    b = oracle.OracleBatch(oracle.TASK_POINTMASS, hi - lo, 2025 + lo)
    b.reset()
    acts = np.random.RandomState(1).uniform(-0.05, 0.05, (T, N, 2))
    obs = np.stack([b.step(acts[t, lo:hi])["obs"] for t in range(T)])  # [T, n_local, 4]
    full = D.gather_rollout(torch.from_numpy(obs))
    t = D.max_over_ranks(float(rank + 1))
    D.barrier()
    if rank == 0:
        q.put((full.numpy(), t))
    torch.distributed.destroy_process_group()


def test_gloo_world2_gather_matches_single_process():
    import torch.multiprocessing as mp

    import oracle

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    full, tmax = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    # single-process reference: identical results for any world size (envs are independent, seeds global)
    N, T = 8, 6
    b = oracle.OracleBatch(oracle.TASK_POINTMASS, N, 2025)
    b.reset()
    acts = np.random.RandomState(1).uniform(-0.05, 0.05, (T, N, 2))
    ref = np.stack([b.step(acts[t])["obs"] for t in range(T)])
    assert full.shape == (T, N, 4) and np.array_equal(full, ref)
    assert tmax == 2.0


def test_bench_gpus2_launches_its_own_ranks():
    """`python bench.py --gpus 2` (the driver's command, no torchrun around it) must fan out to 2 rank processes itself,
    the parent never touching the GPU (the reference's SubprocVecEnv fan-out, scripts/sb3/reach_sac.py:93-96). Run here
    with the --stub stand-in (gloo, CPU, no physics): the launcher, barrier / max-over-ranks timing and the per-chunk
    rollout gather are the real code; the line is marked as a stub."""
    import json
    import subprocess
    import sys

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--stub", "--steps", "5", "--warmup", "1", "--full"],
                         capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["config"]["envs_total"] == 8192 and line["config"]["envs_per_gpu"] == 4096
    assert line["steps"] == 5 and line["warmup"] == 1 and line["scaling"] == "weak" and line["stub"] is True
    g = line["rollout_gather"]
    assert g["chunk_steps"] == 64 and g["shards_bit_identical"] is True and g["backend"] == "gloo"
    assert g["bytes_per_rank"] == 64 * 4096 * 12 * 8
    # a failing rank makes the launcher fail: without --stub the ranks need a GPU, and this host has none
    import torch

    if not torch.cuda.is_available():
        res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "0"],
                             capture_output=True, text=True, timeout=300, env=env)
        assert res.returncode != 0 and "rank" in res.stderr


def test_bench_strong_scaling_mode_splits_a_fixed_env_count():
    """`bench.py --scaling strong --gpus 2`: north_star's "4096 parallel Robot-Reach envs at 1/2/4/8 MI355X" read literally,
    the job's env count stays 4096 and every rank steps 4096 / N of them (the reference's fan-out keeps the env count of the
    job fixed too: scripts/sb3/reach_sac.py:93-96 builds num_envs sub-envs whatever the worker count). Stub ranks, gloo."""
    import json
    import subprocess
    import sys
    import time

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--stub", "--steps", "4", "--warmup", "1", "--scaling", "strong", "--full"],
                         capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["scaling"] == "strong" and line["n_gpus"] == 2
    assert line["config"]["envs_total"] == 4096 and line["config"]["envs_per_gpu"] == 2048
    assert line["rollout_gather"]["bytes_per_rank"] == 64 * 2048 * 12 * 8
    assert abs(line["value"] - 4 * 4096 / (line["ms_per_step"] * 4 * 1e-3)) < 1e-6 * line["value"]
    # an env count the ranks cannot split evenly is refused by every rank, and the launcher reports it at once (it polls all
    # of its children instead of waiting for rank 0's rendezvous to time out)
    t0 = time.time()
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--stub", "--steps", "1", "--warmup", "0", "--scaling", "strong",
                          "--envs-per-gpu", "4097"], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode != 0 and "divisible" in res.stderr and time.time() - t0 < 120


def test_bench_plain_run_is_lean_and_dumps_its_last_step(tmp_path):
    """A plain `bench.py` run carries the headline figures only (what takes runs of its own sits behind --full), and
    --dump-outputs DIR writes what the last timed step returned as float32 / float64 .npy files. Stub env, one process: its
    obs[:, 0] counts the calls of step_flat, so the dump must hold warmup + steps there and nothing stepped it afterwards."""
    import json
    import subprocess
    import sys

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--stub", "--steps", "3", "--warmup", "1", "--envs-per-gpu", "8",
                          "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "env-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert abs(line["value"] - 3 * 8 / (line["ms_per_step"] * 3 * 1e-3)) < 1e-6 * line["value"]
    assert not {"roofline", "rollout_gather", "cpu_baseline", "config1_single_env"} & set(line)
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["fault.npy", "obs.npy"]
    obs, fault = np.load(tmp_path / "out" / "obs.npy"), np.load(tmp_path / "out" / "fault.npy")
    assert obs.dtype == np.float64 and obs.shape == (8, 12) and fault.dtype == np.float32 and fault.shape == (8,)
    assert np.array_equal(obs[:, 0], np.full(8, 4.0)) and not obs[:, 1:].any() and not fault.any()


def test_bench_dump_samples_a_large_output_within_its_budget(tmp_path):
    """Above 64 MB in all, the dump keeps one fixed, seeded sample of envs, the same rows of every array, and says which."""
    import bench

    n = 3000
    big = torch.arange(n, dtype=torch.float64)[:, None].expand(n, 4096).contiguous()  # 98 MB
    small = torch.arange(n, dtype=torch.int32)
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, {"big": big, "small": small})
    a = {p.stem: np.load(p) for p in (tmp_path / "a").iterdir()}
    assert sorted(a) == ["big", "env_index", "small"]
    assert sum(v.nbytes for v in a.values()) <= 64 * 1000 * 1000 and len(a["env_index"]) > n // 2
    assert a["big"].dtype == np.float64 and a["small"].dtype == np.float32
    assert np.array_equal(a["big"][:, 0], a["env_index"]) and np.array_equal(a["small"], a["env_index"]) and np.all(np.diff(a["env_index"]) > 0)
    for k, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / f"{k}.npy"))


def test_lerobot_recorder_schema_and_round_trip(tmp_path):
    """Recorder with the reference collector's conventions (scripts/demonstration_collection.py:39-167): feature names,
    '/' -> '_' key mapping, observation.images.* for image keys, observation.state = concatenated state keys; LeRobot
    v2 directory layout read back with pyarrow."""
    import json
    from collections import OrderedDict

    import pyarrow.parquet as pq

    from mujoco_sim_amd.recording import LeRobotDatasetRecorder
    from mujoco_sim_amd.spaces import Box, Dict

    class FakeEnv:  # the spaces of mujoco_sim/robot_push_button_visual-v0 at 8x8 resolution
        single_observation_space = Dict(OrderedDict([("ur5e/joint_configuration", Box(-np.inf, np.inf, shape=(6,), dtype=np.float64)),
                                                     ("ur5e/Camera/rgb_image", Box(0, 255, shape=(8, 8, 3), dtype=np.uint8)),
                                                     ("Camera/rgb_image", Box(0, 255, shape=(8, 8, 3), dtype=np.uint8))]))
        single_action_space = Box(-3.14, 3.14, shape=(7,), dtype=np.float32)

    rec = LeRobotDatasetRecorder(FakeEnv(), tmp_path / "ds", "test/push_button", fps=10, task="push the button")
    assert set(rec.features) == {"next.reward", "next.success", "seed", "timestamp", "observation.images.ur5e_Camera_rgb_image", "observation.images.Camera_rgb_image",
                                 "ur5e_joint_configuration", "observation.state", "action"}
    assert rec.features["observation.state"]["shape"] == (6,) and rec.features["action"]["shape"] == (7,)
    rs = np.random.RandomState(0)
    N, lengths = 3, [4, 2, 3]
    t = 0
    while rec.n_recorded_episodes < 3:
        obs = {"ur5e/joint_configuration": rs.normal(size=(N, 6)), "ur5e/Camera/rgb_image": rs.randint(0, 255, (N, 8, 8, 3)).astype(np.uint8),
               "Camera/rgb_image": rs.randint(0, 255, (N, 8, 8, 3)).astype(np.uint8)}
        last = np.array([t + 1 == lengths[i] for i in range(N)])
        rec.record_batch(obs, rs.normal(size=(N, 7)), np.arange(N, dtype=float), last, last, seeds=[5, 6, 7])
        t += 1
        if t >= 4:
            break
    rec.finish_recording()
    info = json.loads((tmp_path / "ds" / "meta" / "info.json").read_text())
    assert info["total_episodes"] == 3 and info["total_frames"] == 9 and info["fps"] == 10
    episodes = [json.loads(l) for l in (tmp_path / "ds" / "meta" / "episodes.jsonl").read_text().splitlines()]
    assert sorted(e["length"] for e in episodes) == [2, 3, 4]
    tab = pq.read_table(tmp_path / "ds" / "data" / "chunk-000" / "episode_000000.parquet").to_pydict()
    assert len(tab["action"]) == 2 and len(tab["action"][0]) == 7 and len(tab["observation.images.Camera_rgb_image"][0]) == 8 * 8 * 3  # env 1 ended first
    assert tab["next.success"][-1] == [True] and tab["seed"][0] == [6] and abs(tab["timestamp"][1][0] - 0.1) < 1e-6
    # single-env API of the reference
    rec2 = LeRobotDatasetRecorder(FakeEnv(), tmp_path / "ds2", "test/single", fps=10)
    rec2.start_episode()
    for k in range(3):
        rec2.record({"ur5e/joint_configuration": np.zeros(6), "ur5e/Camera/rgb_image": np.zeros((8, 8, 3), np.uint8), "Camera/rgb_image": np.zeros((8, 8, 3), np.uint8)},
                    np.zeros(7, np.float32), 0.0, k == 2, {})
    rec2.save_episode()
    assert rec2.n_recorded_episodes == 1


def test_gripper_maps_match_the_reference_formulas():
    """mujoco_sim/entities/eef/gripper.py:73-84 on batches: opening <-> driver angle are inverse maps, move() spans ctrl 0..255."""
    import torch

    from mujoco_sim_amd.entities.eef import gripper as g

    d = torch.linspace(0.0, 0.085, 18, dtype=torch.float64)
    th = g.finger_distance_to_joint_angle(d)
    assert torch.allclose(g.joint_angle_to_finger_distance(th), d, atol=1e-15)
    assert abs(float(th[0]) - 0.8) < 1e-15 and abs(float(th[-1])) < 1e-15  # closed: driver at its range end; open: 0
    np.testing.assert_allclose(g.move_ctrl(d).numpy(), np.arcsin((1 - d.numpy() / 0.085) * np.sin(0.8)) / 0.8 * 255, rtol=0, atol=1e-12)
    assert float(g.move_ctrl(torch.tensor([-1.0], dtype=torch.float64))) == 255.0 and float(g.move_ctrl(torch.tensor([1.0], dtype=torch.float64))) == 0.0


def test_registry_and_recorder_match_the_reference_lerobot_configs(tmp_path):
    """SURVEY 8 f-3 / VERDICT r3 item 6: the reference's LeRobot configs (scripts/lerobot/configs/*.yaml, read into
    tests/golden/reference_scene_data.json by make_reference_data_pins.py) state the env interface a trained policy expects:
    task id, fps, episode length, state / action widths, image size, column names. The registered envs and the recorder's feature
    schema equal them; the ONE mismatch is the reference's own (its code names the wrist camera `ur5e/Camera/rgb_image`, its
    YAMLs `ur5e_WristCamera_rgb_image`): the recorder emits the code's key and REFERENCE_YAML_KEY_ALIASES maps it."""
    import json
    from collections import OrderedDict
    from pathlib import Path

    import mujoco_sim_amd as m
    from mujoco_sim_amd.recording import REFERENCE_YAML_KEY_ALIASES, LeRobotDatasetRecorder
    from mujoco_sim_amd.vector_env import TASKS, visual_observation_layout

    pins = json.loads((Path(__file__).parent / "golden" / "reference_scene_data.json").read_text())["lerobot_configs"]
    assert sorted(pins) == ["act_pointmass_reach.yaml", "act_robot_button_push.yaml", "dp_pointmass_reach.yaml", "dp_robot_button_push.yaml"]

    class Space:
        def __init__(self, shape):
            self.shape = tuple(shape)

    class FakeEnv:
        pass

    for name, cfg in pins.items():
        env_id = "mujoco_sim/" + cfg["task"]
        assert env_id in m.registry, env_id
        entry, kw = m.registry[env_id]
        task_name = "point_mass_reach" if "point" in cfg["task"] else "robot_push_button"
        task_cls = m.PointMassReachTask if task_name == "point_mass_reach" else m.RobotPushButtonTask
        assert kw["image_resolution"] == cfg["image_size"]
        assert round(1.0 / task_cls.CONTROL_TIMESTEP) == cfg["fps"]                     # one frame per control step
        assert entry.keywords["max_steps"] == cfg["episode_length"]
        layout = visual_observation_layout(task_name, kw.get("action_type"), kw["image_resolution"])
        env = FakeEnv()
        env.observation_space = OrderedDict((k, Space(shape)) for k, shape, _ in layout)
        assert task_name in TASKS
        act_dim = int(task_cls(**kw).action_spec().shape[0])
        env.action_space = Space((act_dim,))
        assert act_dim == cfg["action_dim"], (name, act_dim)
        rec = LeRobotDatasetRecorder(env, tmp_path / name, "pin/" + name, fps=cfg["fps"])
        assert rec.features["observation.state"]["shape"] == (cfg["state_dim"],)
        assert rec.features["action"]["shape"] == (cfg["action_dim"],)
        emitted = {k: v["shape"] for k, v in rec.features.items() if k.startswith("observation.images.")}
        for key, chw in cfg["image_keys"].items():                                       # LeRobot shapes are channel-first, the env's HWC
            mine = [k for k in emitted if REFERENCE_YAML_KEY_ALIASES.get(k, k) == key]
            assert len(mine) == 1, (name, key, sorted(emitted))
            assert emitted[mine[0]] == (chw[1], chw[2], chw[0])
        assert len(emitted) == len(cfg["image_keys"])
        aliased = LeRobotDatasetRecorder(env, tmp_path / (name + "_a"), "pin/" + name, fps=cfg["fps"], key_aliases=REFERENCE_YAML_KEY_ALIASES)
        assert set(cfg["image_keys"]) <= set(aliased.features)                           # with the aliases the columns ARE the YAML's
        assert set(cfg["stats_keys"]) <= set(aliased.features)
    # the mismatch, spelled out
    assert "observation.images.ur5e_Camera_rgb_image" in {k for k in LeRobotDatasetRecorder.__init__.__globals__["REFERENCE_YAML_KEY_ALIASES"]}
