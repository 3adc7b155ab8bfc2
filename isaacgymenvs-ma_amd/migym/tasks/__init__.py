"""Task map (counterpart of isaacgymenvs/tasks/__init__.py:94-127, restricted to the hot path)."""
from .locomotion import Ant, Humanoid, MAAnt
from .cartpole import Cartpole
from .shadow_hand import ShadowHand
from .franka_reach_ma import FrankaReachMA
from .anymal import Anymal
from .anymal_terrain import AnymalTerrain
from .humanoid_amp import HumanoidAMP
from .quadcopter import Quadcopter

isaacgym_task_map = {
    "Ant": Ant,
    "Humanoid": Humanoid,
    "Cartpole": Cartpole,
    "MAAnt": MAAnt,
    "ShadowHand": ShadowHand,
    "FrankaReachMA": FrankaReachMA,
    "Anymal": Anymal,
    "AnymalTerrain": AnymalTerrain,
    "HumanoidAMP": HumanoidAMP,
    "Quadcopter": Quadcopter,
}
