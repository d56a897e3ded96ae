"""N=1 drop-in for ``envs.RLPickEnv`` (/root/reference/envs/rl_pick_env.py:44-448): same constructor, attributes,
``reset() -> np.float64[9]``, ``step(a) -> (np.float64[9], reward, done, {'is_success': np.float32})`` and the same
consumption of Python's global ``random`` (7 draws per placement try :192-203, 3 unused draws per step :437-439).
The arm pipeline (:310-351) and the reward logic (:358-435) run in the HIP kernels; the gripper and the cube follow the
build's tip-sphere model, not Bullet's finger / cube contact dynamics."""
import math
import random

from .batched import BatchedPickEnv
from .rl_push_env import _HI, _LO, _RLCubeEnv


def draw_pick_placement():
    """Rejection sampling of cube / target positions, rl_pick_env.py:190-208 (<= 1000 tries, last one kept): the cube
    is spawned on the table (z = 0.01; it then settles to ArmEnvConfig.push_rest_z), the target floats anywhere in the workspace box, 0.22 <= 3-D distance <= 0.25."""
    xpos = ypos = xt = yt = zt = 0.0
    for _ in range(1000):
        xpos = random.uniform(_LO[0], _HI[0])
        ypos = random.uniform(_LO[1], _HI[1])
        random.random()                                  # cube yaw :195
        xt = random.uniform(_LO[0], _HI[0])
        yt = random.uniform(_LO[1], _HI[1])
        zt = random.uniform(_LO[2], _HI[2])
        random.random()                                  # target yaw :202
        d = math.sqrt((xpos - xt) ** 2 + (ypos - yt) ** 2 + (0.01 - zt) ** 2)
        if 0.22 <= d <= 0.25:
            break
    return [xpos, ypos, 0.01], [xt, yt, zt]


class RLPickEnv(_RLCubeEnv):
    _Engine = BatchedPickEnv
    _draw_placement = staticmethod(draw_pick_placement)
    _obs_z = 0.257                                       # rl_pick_env.py:94-97

    def __init__(self, is_render=False, is_good_view=False, device="cuda:0"):
        self.gripper_length = self._obs_z                # :79
        self.end_effector_index = 6                      # :101
        super().__init__(is_render, is_good_view, device)

    @property
    def gripper_state(self):
        """0 open, 1 closed, 2 closed and holding the cube (build-defined gripper model)."""
        return int(self._eng.get_state()["aux"][0, 7].item())
