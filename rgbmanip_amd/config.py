"""Default configs with the reference's keys and values (`cfg/controller/rl.yaml`, `cfg/pose_estimator/adapose_*.yaml`).
Hydra is not required: the classes consume plain dicts exactly as `train.py:414-415` hands them over."""
import copy

RL_CONTROLLER_CFG = {
    "name": "rl",
    "controller": {"max_steps": 4, "action_type": "pose", "pose_min": [-0.3, -0.3, 0.4], "pose_max": [0.3, 0.3, 1.0], "early_stop": 4},
    "reward": {"diff_coef": -0.5, "move_success_coef": 8.0, "move_period_coef": -0.0, "far_coef": -2.5, "ori_coef": 0.25,
               "xyz_lookat_coef": -0.05, "bbox_coef": -1.0, "bbox_boundary_coef": -1.0, "have_bbox_coef": 2.0, "center_coef": 12.0,
               "open_coef": 8.0, "view_coef": 0.5, "view_norm_coef": -0.3, "success_coef": 0.0},
    "policy": {"actor_critic_class": "ActorCritic", "pi_hid_sizes": [96, 96, 32], "vf_hid_sizes": [96, 96, 32], "activation": "elu"},
    "learn": {
        "exp_name": "PPO", "reset": True, "num_transitions_per_env": 16, "num_transitions_eval": 512, "num_learning_epochs": 8,
        "num_mini_batches": 4, "clip_range": 0.2, "gamma": 0.98, "lam": 0.98, "init_noise_std": 0.6, "value_loss_coef": 1.0,
        "entropy_coef": 0.0, "learning_rate": 0.00001, "max_grad_norm": 1.0, "use_clipped_value_loss": True,
        "schedule": "adaptive", "desired_kl": 0.016, "max_lr": 0.005, "min_lr": 0.0002, "device": "cuda", "sampler": "sequential",
        "log_dir": "logs/ppo_controller", "save_dir": "saves/ppo_controller", "testing": False, "eval_interval": 64,
        "eval_round": 16, "eval": False, "print_log": True, "contrastive": False, "contrastive_m": 0.99, "asymmetric": False,
    },
    "load": "",
}


# Keys the HIP estimator reads on top of the reference's (INTEGRATION.md section 2 lists them with defaults): hip_dtype, hip_prepare,
# hip_prepare_seed, hip_ransac_seed, hip_upload_chunk, hip_upload ("frames" / "windows": upload whole frames or only their crop windows), hip_view2_heads, hip_graph, hip_graph_max_batch, hip_options, hip_norm_mode,
# hip_dropout, hip_dropout_seed, hip_as_shipped, hip_feature_cache (default False: keep the PSPNet feature map of every frame of the
# controller's view queue across steps; refused together with hip_dropout / hip_as_shipped; "content": the same for estimate() /
# estimate_device(), crops recognised by a device-side fingerprint), hip_feature_cache_records (default 0: two records per pose)
# `name`: "adapose_v5" (every shipped cfg/pose_estimator/*.yaml), "adapose_v4" (train.py:234-236 dispatches it to AdaPoseEstimator_v4) or
# "adapose_baseline" (train.py:242-244: AdaPoseEstimator_baseline, the attention network of lib/network_baseline.py; its checkpoint is a
# StereoPoseNet_with_depth_baseline state dict, with the pose branch only when direct_regression is true; hip_feature_cache, hip_dropout,
# hip_as_shipped and hip_graph are refused for it) or "adapose_realworld" (train.py:246-248: AdaPoseEstimator_realworld, the variance-volume
# network of lib/network_realworld.py with the scaled PnP tail; its checkpoint is v5's plus camera_pts_mlp and a 128-wide pose_mlp1.0;
# direct_regression / use_depth are not read; the four keys above, hip_norm_mode: 1, hip_prepare: host and hip_dtype: fp16 are refused)
# or "adapose_v2" (train.py:226-228: AdaPoseEstimator_v2, the StereoPoseNet of lib/network_v2.py behind a prepare step that draws the points
# at native resolution, with the scaled PnP tail; direct_regression / use_depth are not read; the four keys above, hip_norm_mode: 1,
# hip_prepare: host and hip_upload: windows are refused) or "adapose" (train.py:222-224: AdaPoseEstimator of interface.py, here
# AdaPoseEstimator_v1 - the StereoPoseNet of lib/network.py behind AdaPoseEstimator_v2's prepare step and tail; the same keys are refused)
def adapose_cfg(task_name="one_door_cabinet", checkpoint_path="downloads/pose_estimator/one_door_cabinet.pth", load=True, name="adapose_v5"):
    return {"name": name, "task_name": task_name, "load": load, "checkpoint_path": checkpoint_path, "img_size": 224,
            "use_depth": True, "n_pts": 1024, "direct_regression": True, "real_world": False}


ADAPOSE_CFGS = {
    "adapose_cabinet": adapose_cfg("one_door_cabinet", "downloads/pose_estimator/one_door_cabinet.pth"),
    "adapose_drawer": adapose_cfg("one_drawer_cabinet", "downloads/pose_estimator/one_drawer_cabinet.pth"),
    "adapose_mug": adapose_cfg("mugs", "downloads/pose_estimator/mugs.pth"),
    "adapose_pot": adapose_cfg("pots", "downloads/pose_estimator/pots.pth"),
}


def rl_cfg(task="cabinet", **learn_overrides):
    """cfg/controller/rl.yaml merged with the task name ControlInterface reads (cfg/task/*.yaml `name`)."""
    cfg = copy.deepcopy(RL_CONTROLLER_CFG)
    cfg["learn"].update(learn_overrides)
    cfg["task"] = {"name": task}
    return cfg
