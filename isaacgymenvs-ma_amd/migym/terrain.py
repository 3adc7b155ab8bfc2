"""Terrain generator of the AnymalTerrain task: numpy, on the host, run once at construction.

``Terrain`` restates the reference's class (tasks/anymal_terrain.py:543-673) line for line, but for the triangle mesh:
the physics here takes the heightfield itself (mg_sim_set_heightfield), so
``convert_heightfield_to_trimesh`` is not called and ``slopeTreshold`` is read and ignored.

The sub-terrain functions the class calls (``isaacgym.terrain_utils`` in the reference's imports) are not part of the
reference tree.  The ones below are written from their definitions and claim no parity with NVIDIA's:
a seed gives the same terrain on every run here, not the terrain Isaac Gym would build from it.  Every function works
on ``SubTerrain.height_field_raw`` in place; sizes in metres become ``int(x / horizontal_scale)`` cells, heights
``int(h / vertical_scale)`` units; every draw comes from ``np.random``'s global state, so ``np.random.seed`` fixes a
terrain.
"""
from __future__ import annotations

import numpy as np


class SubTerrain:
    def __init__(self, terrain_name="terrain", width=256, length=256, vertical_scale=1.0, horizontal_scale=1.0):
        self.terrain_name = terrain_name
        self.vertical_scale = vertical_scale
        self.horizontal_scale = horizontal_scale
        self.width = width
        self.length = length
        self.height_field_raw = np.zeros((self.width, self.length), dtype=np.int16)


def _platform(t, platform_size):
    """the index ranges of the central square of side int(platform_size / hs) cells"""
    p = int(platform_size / t.horizontal_scale)
    x1, y1 = (t.width - p) // 2, (t.length - p) // 2
    return slice(x1, x1 + p), slice(y1, y1 + p)


def pyramid_sloped_terrain(t, slope, platform_size=1.):
    """a pyramid of the given slope (negative: a pit) with a flat top: the product of two tents, clipped at the height
    it has at the platform's corner"""
    cx, cy = t.width / 2, t.length / 2
    x, y = np.arange(t.width).reshape(-1, 1), np.arange(t.length).reshape(1, -1)
    xx = (cx - np.abs(cx - x)) / cx
    yy = (cy - np.abs(cy - y)) / cy
    max_height = int(slope * (t.horizontal_scale / t.vertical_scale) * (t.width / 2))
    t.height_field_raw += (max_height * xx * yy).astype(t.height_field_raw.dtype)
    p = int(platform_size / t.horizontal_scale / 2)
    h_p = t.height_field_raw[t.width // 2 - p, t.length // 2 - p]
    t.height_field_raw = np.clip(t.height_field_raw, min(h_p, 0), max(h_p, 0)).astype(np.int16)
    return t


def pyramid_stairs_terrain(t, step_width, step_height, platform_size=1.):
    """concentric square rings, each one step higher (negative step_height: lower) than the ring around it"""
    sw = int(step_width / t.horizontal_scale)
    sh = int(step_height / t.vertical_scale)
    p = int(platform_size / t.horizontal_scale)
    height, x0, x1, y0, y1 = 0, 0, t.width, 0, t.length
    while (x1 - x0) > p and (y1 - y0) > p:
        x0, x1, y0, y1 = x0 + sw, x1 - sw, y0 + sw, y1 - sw
        height += sh
        t.height_field_raw[x0:x1, y0:y1] = height
    return t


def discrete_obstacles_terrain(t, max_height, min_size, max_size, num_rects, platform_size=1.):
    """num_rects rectangles of a height from {-H, -H/2, H/2, H}, then a flat central platform"""
    H = int(max_height / t.vertical_scale)
    lo, hi = int(min_size / t.horizontal_scale), int(max_size / t.horizontal_scale)
    rows, cols = t.height_field_raw.shape
    heights = [-H, -H // 2, H // 2, H]
    sides = range(lo, hi, 4)
    for _ in range(num_rects):
        w, l = np.random.choice(sides), np.random.choice(sides)
        i = np.random.choice(range(0, rows - w, 4))
        j = np.random.choice(range(0, cols - l, 4))
        t.height_field_raw[i:i + w, j:j + l] = np.random.choice(heights)
    t.height_field_raw[_platform(t, platform_size)] = 0
    return t


def random_uniform_terrain(t, min_height, max_height, step=1, downsampled_scale=None):
    """heights drawn on a coarse grid of pitch downsampled_scale, interpolated bilinearly to the full grid, rounded
    and added"""
    if downsampled_scale is None:
        downsampled_scale = t.horizontal_scale
    lo, hi = int(min_height / t.vertical_scale), int(max_height / t.vertical_scale)
    st = int(step / t.vertical_scale)
    values = np.arange(lo, hi + st, st)
    nw = int(t.width * t.horizontal_scale / downsampled_scale)
    nl = int(t.length * t.horizontal_scale / downsampled_scale)
    coarse = np.random.choice(values, (nw, nl)).astype(np.float64)
    xc, yc = np.linspace(0, t.width * t.horizontal_scale, nw), np.linspace(0, t.length * t.horizontal_scale, nl)
    xf, yf = np.linspace(0, t.width * t.horizontal_scale, t.width), np.linspace(0, t.length * t.horizontal_scale, t.length)
    # bilinear on a rectilinear grid: linear along x, then along y
    along_x = np.stack([np.interp(xf, xc, coarse[:, j]) for j in range(nl)], axis=1)
    full = np.stack([np.interp(yf, yc, along_x[i]) for i in range(t.width)], axis=0)
    t.height_field_raw += np.rint(full).astype(np.int16)
    return t


def stepping_stones_terrain(t, stone_size, stone_distance, max_height, platform_size=1., depth=-10):
    """a pit of the given depth with square stones of random height in [-max_height, max_height], a fixed gap apart,
    and a flat central platform"""
    ss = max(int(stone_size / t.horizontal_scale), 1)
    sd = int(stone_distance / t.horizontal_scale)
    mh = int(max_height / t.vertical_scale)
    heights = np.arange(-mh, mh + 1)
    t.height_field_raw[:, :] = int(depth / t.vertical_scale)
    for x0 in range(0, t.width, ss + sd):
        for y0 in range(0, t.length, ss + sd):
            t.height_field_raw[x0:x0 + ss, y0:y0 + ss] = np.random.choice(heights)
    t.height_field_raw[_platform(t, platform_size)] = 0
    return t


class Terrain:
    def __init__(self, cfg, num_robots) -> None:
        self.type = cfg["terrainType"]
        if self.type in ["none", "plane"]:
            return
        self.horizontal_scale = 0.1
        self.vertical_scale = 0.005
        self.border_size = 20
        self.num_per_env = 2
        self.env_length = cfg["mapLength"]
        self.env_width = cfg["mapWidth"]
        self.proportions = [np.sum(cfg["terrainProportions"][:i + 1]) for i in range(len(cfg["terrainProportions"]))]

        self.env_rows = cfg["numLevels"]
        self.env_cols = cfg["numTerrains"]
        self.num_maps = self.env_rows * self.env_cols
        self.num_per_env = int(num_robots / self.num_maps)
        self.env_origins = np.zeros((self.env_rows, self.env_cols, 3))

        self.width_per_env_pixels = int(self.env_width / self.horizontal_scale)
        self.length_per_env_pixels = int(self.env_length / self.horizontal_scale)

        self.border = int(self.border_size / self.horizontal_scale)
        self.tot_cols = int(self.env_cols * self.width_per_env_pixels) + 2 * self.border
        self.tot_rows = int(self.env_rows * self.length_per_env_pixels) + 2 * self.border

        self.height_field_raw = np.zeros((self.tot_rows, self.tot_cols), dtype=np.int16)
        if cfg["curriculum"]:
            self.curiculum(num_robots, num_terrains=self.env_cols, num_levels=self.env_rows)
        else:
            self.randomized_terrain()
        self.heightsamples = self.height_field_raw
        self.slope_treshold = cfg.get("slopeTreshold")   # the mesh's: read and ignored (no mesh is built)

    def _place(self, terrain, i, j):
        """the sub-terrain into the field at map (i, j), and the map's origin (anymal_terrain.py:655-673)"""
        start_x = self.border + i * self.length_per_env_pixels
        end_x = self.border + (i + 1) * self.length_per_env_pixels
        start_y = self.border + j * self.width_per_env_pixels
        end_y = self.border + (j + 1) * self.width_per_env_pixels
        self.height_field_raw[start_x: end_x, start_y:end_y] = terrain.height_field_raw

        env_origin_x = (i + 0.5) * self.env_length
        env_origin_y = (j + 0.5) * self.env_width
        x1 = int((self.env_length / 2. - 1) / self.horizontal_scale)
        x2 = int((self.env_length / 2. + 1) / self.horizontal_scale)
        y1 = int((self.env_width / 2. - 1) / self.horizontal_scale)
        y2 = int((self.env_width / 2. + 1) / self.horizontal_scale)
        env_origin_z = np.max(terrain.height_field_raw[x1:x2, y1:y2]) * self.vertical_scale
        self.env_origins[i, j] = [env_origin_x, env_origin_y, env_origin_z]

    def _sub_terrain(self):
        return SubTerrain("terrain", width=self.width_per_env_pixels, length=self.width_per_env_pixels,
                          vertical_scale=self.vertical_scale, horizontal_scale=self.horizontal_scale)

    def randomized_terrain(self):
        for k in range(self.num_maps):
            (i, j) = np.unravel_index(k, (self.env_rows, self.env_cols))
            terrain = self._sub_terrain()
            choice = np.random.uniform(0, 1)
            if choice < 0.1:
                if np.random.choice([0, 1]):
                    pyramid_sloped_terrain(terrain, np.random.choice([-0.3, -0.2, 0, 0.2, 0.3]))
                    random_uniform_terrain(terrain, min_height=-0.1, max_height=0.1, step=0.05, downsampled_scale=0.2)
                else:
                    pyramid_sloped_terrain(terrain, np.random.choice([-0.3, -0.2, 0, 0.2, 0.3]))
            elif choice < 0.6:
                step_height = np.random.choice([-0.15, 0.15])
                pyramid_stairs_terrain(terrain, step_width=0.31, step_height=step_height, platform_size=3.)
            elif choice < 1.:
                discrete_obstacles_terrain(terrain, 0.15, 1., 2., 40, platform_size=3.)
            self._place(terrain, i, j)

    def curiculum(self, num_robots, num_terrains, num_levels):
        for j in range(num_terrains):
            for i in range(num_levels):
                terrain = self._sub_terrain()
                difficulty = i / num_levels
                choice = j / num_terrains

                slope = difficulty * 0.4
                step_height = 0.05 + 0.175 * difficulty
                discrete_obstacles_height = 0.025 + difficulty * 0.15
                stepping_stones_size = 2 - 1.8 * difficulty
                if choice < self.proportions[0]:
                    if choice < 0.05:
                        slope *= -1
                    pyramid_sloped_terrain(terrain, slope=slope, platform_size=3.)
                elif choice < self.proportions[1]:
                    if choice < 0.15:
                        slope *= -1
                    pyramid_sloped_terrain(terrain, slope=slope, platform_size=3.)
                    random_uniform_terrain(terrain, min_height=-0.1, max_height=0.1, step=0.025, downsampled_scale=0.2)
                elif choice < self.proportions[3]:
                    if choice < self.proportions[2]:
                        step_height *= -1
                    pyramid_stairs_terrain(terrain, step_width=0.31, step_height=step_height, platform_size=3.)
                elif choice < self.proportions[4]:
                    discrete_obstacles_terrain(terrain, discrete_obstacles_height, 1., 2., 40, platform_size=3.)
                else:
                    stepping_stones_terrain(terrain, stone_size=stepping_stones_size, stone_distance=0.1, max_height=0.,
                                            platform_size=3.)
                self._place(terrain, i, j)
