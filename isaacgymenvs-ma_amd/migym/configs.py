"""Task configuration defaults and the hydra-free resolver.

The reference composes ``cfg/config.yaml`` + ``cfg/task/<Task>.yaml`` with
hydra/OmegaConf and four custom resolvers (isaacgymenvs/__init__.py:8-11,
35-38).  Neither hydra nor omegaconf is available here, so the values the hot
path reads are restated as plain dicts (same keys, so ``cfg['env'][...]``
overrides written for the reference work unchanged) and interpolations are
resolved eagerly by :func:`task_config`.

Sources of the values: cfg/config.yaml:18-32 (devices, physx threads,
solver), cfg/task/Ant.yaml, Humanoid.yaml, Cartpole.yaml, ShadowHand.yaml.
"""
from __future__ import annotations

import copy
import math

ROOT_DEFAULTS = {
    "physics_engine": "physx",
    "pipeline": "gpu",
    "sim_device": "cuda:0",
    "rl_device": "cuda:0",
    "graphics_device_id": 0,
    "num_threads": 4,
    "solver_type": 1,       # reference default TGS; this build implements PGS
    "num_subscenes": 4,
    "seed": 42,
}

_PHYSX_COMMON = {
    "num_threads": 4, "solver_type": 1, "use_gpu": True, "num_position_iterations": 4,
    "num_velocity_iterations": 0, "contact_offset": 0.02, "rest_offset": 0.0,
    "bounce_threshold_velocity": 0.2, "max_depenetration_velocity": 10.0,
    "default_buffer_size_multiplier": 5.0, "max_gpu_contact_pairs": 8 * 1024 * 1024,
    "num_subscenes": 4, "contact_collection": 0,
}


def _sim(dt=0.0166, **physx):
    p = dict(_PHYSX_COMMON)
    p.update(physx)
    return {"dt": dt, "substeps": 2, "up_axis": "z", "use_gpu_pipeline": True,
            "gravity": [0.0, 0.0, -9.81], "physx": p}


_LOCO_PLANE = {"staticFriction": 1.0, "dynamicFriction": 1.0, "restitution": 0.0}


# task.randomization_params of the task YAMLs (cfg/task/Ant.yaml:63-101, Humanoid.yaml:63-129,
# ShadowHand.yaml:64-169); applied when task.randomize is True (migym/dr.py)
_DR_ANT = {'frequency': 600,
 'observations': {'range': [0, 0.002], 'operation': 'additive', 'distribution': 'gaussian'},
 'actions': {'range': [0.0, 0.02], 'operation': 'additive', 'distribution': 'gaussian'},
 'actor_params': {'ant': {'color': True,
                          'rigid_body_properties': {'mass': {'range': [0.5, 1.5],
                                                             'operation': 'scaling',
                                                             'distribution': 'uniform',
                                                             'setup_only': True}},
                          'dof_properties': {'damping': {'range': [0.5, 1.5],
                                                         'operation': 'scaling',
                                                         'distribution': 'uniform'},
                                             'stiffness': {'range': [0.5, 1.5],
                                                           'operation': 'scaling',
                                                           'distribution': 'uniform'},
                                             'lower': {'range': [0, 0.01],
                                                       'operation': 'additive',
                                                       'distribution': 'gaussian'},
                                             'upper': {'range': [0, 0.01],
                                                       'operation': 'additive',
                                                       'distribution': 'gaussian'}}}}}
_DR_HUMANOID = {'frequency': 600,
 'observations': {'range': [0, 0.002], 'operation': 'additive', 'distribution': 'gaussian'},
 'actions': {'range': [0.0, 0.02], 'operation': 'additive', 'distribution': 'gaussian'},
 'sim_params': {'gravity': {'range': [0, 0.4],
                            'operation': 'additive',
                            'distribution': 'gaussian',
                            'schedule': 'linear',
                            'schedule_steps': 3000}},
 'actor_params': {'humanoid': {'color': True,
                               'rigid_body_properties': {'mass': {'range': [0.5, 1.5],
                                                                  'operation': 'scaling',
                                                                  'distribution': 'uniform',
                                                                  'setup_only': True,
                                                                  'schedule': 'linear',
                                                                  'schedule_steps': 3000}},
                               'rigid_shape_properties': {'friction': {'num_buckets': 500,
                                                                       'range': [0.7, 1.3],
                                                                       'operation': 'scaling',
                                                                       'distribution': 'uniform',
                                                                       'schedule': 'linear',
                                                                       'schedule_steps': 3000},
                                                          'restitution': {'range': [0.0, 0.7],
                                                                          'operation': 'scaling',
                                                                          'distribution': 'uniform',
                                                                          'schedule': 'linear',
                                                                          'schedule_steps': 3000}},
                               'dof_properties': {'damping': {'range': [0.5, 1.5],
                                                              'operation': 'scaling',
                                                              'distribution': 'uniform',
                                                              'schedule': 'linear',
                                                              'schedule_steps': 3000},
                                                  'stiffness': {'range': [0.5, 1.5],
                                                                'operation': 'scaling',
                                                                'distribution': 'uniform',
                                                                'schedule': 'linear',
                                                                'schedule_steps': 3000},
                                                  'lower': {'range': [0, 0.01],
                                                            'operation': 'additive',
                                                            'distribution': 'gaussian',
                                                            'schedule': 'linear',
                                                            'schedule_steps': 3000},
                                                  'upper': {'range': [0, 0.01],
                                                            'operation': 'additive',
                                                            'distribution': 'gaussian',
                                                            'schedule': 'linear',
                                                            'schedule_steps': 3000}}}}}
_DR_SHADOWHAND = {'frequency': 720,
 'observations': {'range': [0, 0.002],
                  'range_correlated': [0, 0.001],
                  'operation': 'additive',
                  'distribution': 'gaussian'},
 'actions': {'range': [0.0, 0.05],
             'range_correlated': [0, 0.015],
             'operation': 'additive',
             'distribution': 'gaussian'},
 'sim_params': {'gravity': {'range': [0, 0.4], 'operation': 'additive', 'distribution': 'gaussian'}},
 'actor_params': {'hand': {'color': True,
                           'tendon_properties': {'damping': {'range': [0.3, 3.0],
                                                             'operation': 'scaling',
                                                             'distribution': 'loguniform'},
                                                 'stiffness': {'range': [0.75, 1.5],
                                                               'operation': 'scaling',
                                                               'distribution': 'loguniform'}},
                           'dof_properties': {'damping': {'range': [0.3, 3.0],
                                                          'operation': 'scaling',
                                                          'distribution': 'loguniform'},
                                              'stiffness': {'range': [0.75, 1.5],
                                                            'operation': 'scaling',
                                                            'distribution': 'loguniform'},
                                              'lower': {'range': [0, 0.01],
                                                        'operation': 'additive',
                                                        'distribution': 'gaussian'},
                                              'upper': {'range': [0, 0.01],
                                                        'operation': 'additive',
                                                        'distribution': 'gaussian'}},
                           'rigid_body_properties': {'mass': {'range': [0.5, 1.5],
                                                              'operation': 'scaling',
                                                              'distribution': 'uniform',
                                                              'setup_only': True}},
                           'rigid_shape_properties': {'friction': {'num_buckets': 250,
                                                                   'range': [0.7, 1.3],
                                                                   'operation': 'scaling',
                                                                   'distribution': 'uniform'}}},
                  'object': {'scale': {'range': [0.95, 1.05],
                                       'operation': 'scaling',
                                       'distribution': 'uniform',
                                       'setup_only': True},
                             'rigid_body_properties': {'mass': {'range': [0.5, 1.5],
                                                                'operation': 'scaling',
                                                                'distribution': 'uniform',
                                                                'setup_only': True}},
                             'rigid_shape_properties': {'friction': {'num_buckets': 250,
                                                                     'range': [0.7, 1.3],
                                                                     'operation': 'scaling',
                                                                     'distribution': 'uniform'}}}}}

TASKS = {
    "Ant": {
        "name": "Ant",
        "env": {
            "numEnvs": 4096, "envSpacing": 5, "episodeLength": 1000, "enableDebugVis": False,
            "clipActions": 1.0, "powerScale": 1.0, "controlFrequencyInv": 1,
            "headingWeight": 0.5, "upWeight": 0.1, "actionsCost": 0.005, "energyCost": 0.05,
            "dofVelocityScale": 0.2, "contactForceScale": 0.1, "jointsAtLimitCost": 0.1,
            "deathCost": -2.0, "terminationHeight": 0.31, "plane": dict(_LOCO_PLANE),
            "asset": {"assetFileName": "mjcf/nv_ant.xml"}, "enableCameraSensors": False,
        },
        "sim": _sim(),
        "task": {"randomize": False, "randomization_params": _DR_ANT},
    },
    "Humanoid": {
        "name": "Humanoid",
        "env": {
            "numEnvs": 4096, "envSpacing": 5, "episodeLength": 1000, "enableDebugVis": False,
            "clipActions": 1.0, "powerScale": 1.0, "headingWeight": 0.5, "upWeight": 0.1,
            "actionsCost": 0.01, "energyCost": 0.05, "dofVelocityScale": 0.1, "angularVelocityScale": 0.25,
            "contactForceScale": 0.01, "jointsAtLimitCost": 0.25, "deathCost": -1.0,
            "terminationHeight": 0.8, "asset": {"assetFileName": "mjcf/nv_humanoid.xml"},
            "plane": dict(_LOCO_PLANE), "enableCameraSensors": False,
        },
        "sim": _sim(),
        "task": {"randomize": False, "randomization_params": _DR_HUMANOID},
    },
    "Cartpole": {
        "name": "Cartpole",
        "env": {
            "numEnvs": 512, "envSpacing": 4.0, "resetDist": 3.0, "maxEffort": 400.0,
            "clipObservations": 5.0, "clipActions": 1.0,
            "asset": {"assetRoot": "../../assets", "assetFileName": "urdf/cartpole.urdf"},
            "enableCameraSensors": False,
        },
        "sim": _sim(rest_offset=0.001, max_depenetration_velocity=100.0, default_buffer_size_multiplier=2.0,
                    max_gpu_contact_pairs=1024 * 1024),
        "task": {"randomize": False},
    },
}

TASKS["ShadowHand"] = {
    "name": "ShadowHand",
    "env": {
        "numEnvs": 16384, "envSpacing": 0.75, "episodeLength": 600, "enableDebugVis": False, "aggregateMode": 1,
        "clipObservations": 5.0, "clipActions": 1.0, "stiffnessScale": 1.0, "forceLimitScale": 1.0,
        "useRelativeControl": False, "dofSpeedScale": 20.0, "actionsMovingAverage": 1.0,
        "controlFrequencyInv": 1, "startPositionNoise": 0.01, "startRotationNoise": 0.0,
        "resetPositionNoise": 0.01, "resetRotationNoise": 0.0, "resetDofPosRandomInterval": 0.2,
        "resetDofVelRandomInterval": 0.0, "forceScale": 0.0, "forceProbRange": [0.001, 0.1],
        "forceDecay": 0.99, "forceDecayInterval": 0.08, "distRewardScale": -10.0, "rotRewardScale": 1.0,
        "rotEps": 0.1, "actionPenaltyScale": -0.0002, "reachGoalBonus": 250, "fallDistance": 0.24,
        "fallPenalty": 0.0, "objectType": "block", "observationType": "full_state",
        "asymmetric_observations": False, "successTolerance": 0.1, "printNumSuccesses": False,
        "maxConsecutiveSuccesses": 0,
        "asset": {"assetFileName": "mjcf/open_ai_assets/hand/shadow_hand.xml",
                  "assetFileNameBlock": "urdf/objects/cube_multicolor.urdf",
                  "assetFileNameEgg": "mjcf/open_ai_assets/hand/egg.xml",
                  "assetFileNamePen": "mjcf/open_ai_assets/hand/pen.xml"},
        "enableCameraSensors": False,
    },
    "sim": _sim(dt=0.01667, num_position_iterations=8, contact_offset=0.002, rest_offset=0.0,
                bounce_threshold_velocity=0.2, max_depenetration_velocity=1000.0),
    "task": {"randomize": False, "randomization_params": _DR_SHADOWHAND},
}

# Multi-agent Ant (build-defined, SURVEY.md §8(a) row A-MA): A ant actors per env.
TASKS["MAAnt"] = copy.deepcopy(TASKS["Ant"])
TASKS["MAAnt"]["name"] = "MAAnt"
TASKS["MAAnt"]["env"].update({"numAgents": 4, "agentSpacing": 2.0})

# FrankaReachMA (the fork's multi-arm reach task, cfg/task/FrankaReachMA.yaml): only the keys the task reads.  No
# Franka asset is shipped: env.asset.modelTable names a JSON model table (tools/build_models.py franka_panda writes
# one), or assetRoot + assetFileNameFranka a URDF.
TASKS["FrankaReachMA"] = {
    "name": "FrankaReachMA",
    "env": {
        "numEnvs": 8192, "numAgents": 2, "numTargets": -1, "episodeLength": 150,
        "clipObservations": 5.0, "clipActions": 1.0, "startPositionNoise": 0.25, "startRotationNoise": 0.785,
        "frankaPositionNoise": 0.0, "frankaRotationNoise": 0.0, "frankaDofNoise": 0.25, "actionScale": 1.0,
        "controlType": "osc", "controlFrequencyInv": 1,
        "asset": {"assetRoot": "../../assets",
                  "assetFileNameFranka": "urdf/franka_description/robots/franka_panda_gripper.urdf"},
    },
    "sim": _sim(dt=0.01667, num_position_iterations=8, num_velocity_iterations=1, contact_offset=0.005,
                rest_offset=0.0, bounce_threshold_velocity=0.2, max_depenetration_velocity=1000.0),
    "task": {"randomize": False},
}

# Anymal (cfg/task/Anymal.yaml): only the keys the task reads.  No ANYmal asset is shipped: env.asset.modelTable names
# a JSON model table (tools/build_models.py anymal_c writes one), or assetRoot + assetFileName the URDF.
TASKS["Anymal"] = {
    "name": "Anymal",
    "env": {
        "numEnvs": 4096, "envSpacing": 4.0, "clipObservations": 5.0, "clipActions": 1.0,
        "plane": dict(_LOCO_PLANE),
        "baseInitState": {"pos": [0.0, 0.0, 0.62], "rot": [0.0, 0.0, 0.0, 1.0], "vLinear": [0.0, 0.0, 0.0],
                          "vAngular": [0.0, 0.0, 0.0]},
        "randomCommandVelocityRanges": {"linear_x": [-2.0, 2.0], "linear_y": [-1.0, 1.0], "yaw": [-1.0, 1.0]},
        "control": {"stiffness": 85.0, "damping": 2.0, "actionScale": 0.5, "controlFrequencyInv": 1},
        "defaultJointAngles": {"LF_HAA": 0.03, "LH_HAA": 0.03, "RF_HAA": -0.03, "RH_HAA": -0.03,
                               "LF_HFE": 0.4, "LH_HFE": -0.4, "RF_HFE": 0.4, "RH_HFE": -0.4,
                               "LF_KFE": -0.8, "LH_KFE": 0.8, "RF_KFE": -0.8, "RH_KFE": 0.8},
        "urdfAsset": {"collapseFixedJoints": True, "fixBaseLink": False, "defaultDofDriveMode": 4},
        "learn": {"linearVelocityXYRewardScale": 1.0, "angularVelocityZRewardScale": 0.5,
                  "torqueRewardScale": -0.000025, "linearVelocityScale": 2.0, "angularVelocityScale": 0.25,
                  "dofPositionScale": 1.0, "dofVelocityScale": 0.05, "episodeLength_s": 50},
        "asset": {"assetRoot": "../../assets", "assetFileName": "urdf/anymal_c/urdf/anymal.urdf"},
        "enableCameraSensors": False,
    },
    "sim": _sim(dt=0.02, num_position_iterations=4, num_velocity_iterations=1, contact_offset=0.02, rest_offset=0.0,
                bounce_threshold_velocity=0.2, max_depenetration_velocity=100.0, contact_collection=1),
    "task": {"randomize": False},
}


# AnymalTerrain (cfg/task/AnymalTerrain.yaml): only the keys the task reads.  The model is found as Anymal's is:
# env.asset.modelTable names a JSON model table (tools/build_models.py anymal_minimal writes one), or assetRoot +
# assetFileName the URDF.  frictionRange is kept for the record: per-env friction is not built.
TASKS["AnymalTerrain"] = {
    "name": "AnymalTerrain",
    "env": {
        # no clipObservations / clipActions: the reference's YAML has neither, so VecTask clips at infinity
        "numEnvs": 4096, "envSpacing": 3.0, "enableDebugVis": False,
        "terrain": {"terrainType": "trimesh", "staticFriction": 1.0, "dynamicFriction": 1.0, "restitution": 0.0,
                    "curriculum": True, "maxInitMapLevel": 0, "mapLength": 8.0, "mapWidth": 8.0, "numLevels": 10,
                    "numTerrains": 20, "terrainProportions": [0.1, 0.1, 0.35, 0.25, 0.2], "slopeTreshold": 0.5},
        "baseInitState": {"pos": [0.0, 0.0, 0.62], "rot": [0.0, 0.0, 0.0, 1.0], "vLinear": [0.0, 0.0, 0.0],
                          "vAngular": [0.0, 0.0, 0.0]},
        "randomCommandVelocityRanges": {"linear_x": [-1.0, 1.0], "linear_y": [-1.0, 1.0], "yaw": [-3.14, 3.14]},
        "control": {"stiffness": 80.0, "damping": 2.0, "actionScale": 0.5, "decimation": 4},
        "defaultJointAngles": {"LF_HAA": 0.03, "LH_HAA": 0.03, "RF_HAA": -0.03, "RH_HAA": -0.03,
                               "LF_HFE": 0.4, "LH_HFE": -0.4, "RF_HFE": 0.4, "RH_HFE": -0.4,
                               "LF_KFE": -0.8, "LH_KFE": 0.8, "RF_KFE": -0.8, "RH_KFE": 0.8},
        "urdfAsset": {"file": "urdf/anymal_c/urdf/anymal_minimal.urdf", "footName": "SHANK", "kneeName": "THIGH",
                      "collapseFixedJoints": True, "fixBaseLink": False, "defaultDofDriveMode": 4},
        "learn": {"allowKneeContacts": True, "terminalReward": 0.0, "linearVelocityXYRewardScale": 1.0,
                  "linearVelocityZRewardScale": -4.0, "angularVelocityXYRewardScale": -0.05,
                  "angularVelocityZRewardScale": 0.5, "orientationRewardScale": -0.0, "torqueRewardScale": -0.00002,
                  "jointAccRewardScale": -0.0005, "baseHeightRewardScale": -0.0, "feetAirTimeRewardScale": 1.0,
                  "kneeCollisionRewardScale": -0.25, "feetStumbleRewardScale": -0.0, "actionRateRewardScale": -0.01,
                  "hipRewardScale": -0.0, "linearVelocityScale": 2.0, "angularVelocityScale": 0.25,
                  "dofPositionScale": 1.0, "dofVelocityScale": 0.05, "heightMeasurementScale": 5.0,
                  "addNoise": True, "noiseLevel": 1.0, "dofPositionNoise": 0.01, "dofVelocityNoise": 1.5,
                  "linearVelocityNoise": 0.1, "angularVelocityNoise": 0.2, "gravityNoise": 0.05,
                  "heightMeasurementNoise": 0.06, "randomizeFriction": True, "frictionRange": [0.5, 1.25],
                  "pushRobots": True, "pushInterval_s": 15, "episodeLength_s": 20},
        "asset": {"assetRoot": "../../assets", "assetFileName": "urdf/anymal_c/urdf/anymal_minimal.urdf"},
        "enableCameraSensors": False,
    },
    "sim": _sim(dt=0.005, num_position_iterations=4, num_velocity_iterations=1, contact_offset=0.02, rest_offset=0.0,
                bounce_threshold_velocity=0.2, max_depenetration_velocity=100.0, contact_collection=1),
    "task": {"randomize": False},
}
TASKS["AnymalTerrain"]["sim"]["substeps"] = 1


# HumanoidAMP (cfg/task/HumanoidAMP.yaml): only the keys the task reads.  Neither the AMP humanoid nor a motion clip is
# shipped: env.asset.modelTable names a JSON model table (tools/build_models.py amp_humanoid writes one), or assetRoot +
# assetFileName the MJCF; env.motion_file names a clip (.npy / .npz / .yaml), absolute or under env.asset.motionRoot.
TASKS["HumanoidAMP"] = {
    "name": "HumanoidAMP",
    "env": {
        "numEnvs": 4096, "envSpacing": 5, "episodeLength": 300, "cameraFollow": True, "enableDebugVis": False,
        "pdControl": True, "powerScale": 1.0, "controlFrequencyInv": 2, "stateInit": "Random", "hybridInitProb": 0.5,
        "numAMPObsSteps": 2, "localRootObs": False, "contactBodies": ["right_foot", "left_foot"],
        "terminationHeight": 0.5, "enableEarlyTermination": True,
        "motion_file": "amp_humanoid_run.npy",
        "asset": {"assetRoot": "../../assets", "assetFileName": "mjcf/amp_humanoid.xml",
                  "motionRoot": "../../assets/amp/motions"},
        "plane": dict(_LOCO_PLANE),
    },
    "sim": _sim(dt=0.0166, num_position_iterations=4, num_velocity_iterations=0, contact_offset=0.02, rest_offset=0.0,
                bounce_threshold_velocity=0.2, max_depenetration_velocity=10.0, contact_collection=2),
    "task": {"randomize": False},
}

# Quadcopter (cfg/task/Quadcopter.yaml).  The reference writes its own MJCF at run time; migym builds the model from
# the same dimensions (migym.model.quadcopter_model), so the task needs no asset.
TASKS["Quadcopter"] = {
    "name": "Quadcopter",
    "env": {"numEnvs": 8192, "envSpacing": 1.25, "maxEpisodeLength": 500, "enableDebugVis": False,
            "clipObservations": 5.0, "clipActions": 1.0, "enableCameraSensors": False},
    "sim": _sim(dt=0.01, num_position_iterations=4, num_velocity_iterations=0, contact_offset=0.02, rest_offset=0.001,
                bounce_threshold_velocity=0.2, max_depenetration_velocity=1000.0, contact_collection=0),
    "task": {"randomize": False},
}


def resolve_default(default, arg):
    """``${resolve_default:d,x}`` (isaacgymenvs/__init__.py:11)."""
    return default if arg in ("", None) else arg


def task_config(task: str, num_envs=None, sim_device="cuda:0", pipeline="gpu", overrides=None) -> dict:
    """cfg.task as a plain dict with interpolations resolved (``omegaconf_to_dict``)."""
    if task not in TASKS:
        raise ValueError(f"unknown task {task!r}; available: {sorted(TASKS)}")
    cfg = copy.deepcopy(TASKS[task])
    cfg["physics_engine"] = ROOT_DEFAULTS["physics_engine"]
    cfg["env"]["numEnvs"] = resolve_default(cfg["env"]["numEnvs"], num_envs)
    cfg["sim"]["use_gpu_pipeline"] = pipeline.lower() == "gpu"                   # ${eq:${...pipeline},"gpu"}
    cfg["sim"]["physx"]["use_gpu"] = "cuda" in sim_device.lower()                 # ${contains:"cuda",...}
    for k, v in (overrides or {}).items():
        node = cfg
        parts = k.split(".")
        for p in parts[:-1]:
            node = node.setdefault(p, {})
        node[parts[-1]] = v
    return cfg


def clip_value(cfg_env, key):
    v = cfg_env.get(key, math.inf)
    return float(v)
