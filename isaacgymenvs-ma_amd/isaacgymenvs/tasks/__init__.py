from migym.tasks import isaacgym_task_map, Ant, Humanoid, Cartpole, FrankaReachMA, Anymal, \
    HumanoidAMP, Quadcopter  # noqa: F401
