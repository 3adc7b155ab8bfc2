from migym.tasks import isaacgym_task_map, Ant, Humanoid, Cartpole, FrankaReachMA, Anymal, \
    HumanoidAMP, Quadcopter, AnymalTerrain  # noqa: F401
