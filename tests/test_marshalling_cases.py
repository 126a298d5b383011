"""The marshalling helpers under the Python surface, case by case: what each `_c_*` helper of SimulationHandler makes of an
input -- the fields of the records it fills, read back from the struct array, or the exact text of the EggError it raises --
and what the getters make of a struct array filled by hand.  Every table is literal; a value is compared by its repr, so
that nan equals nan and -0.0 differs from 0.0.  No device."""
import ctypes as C

import pytest

from egg_fluid_simulation_amd import EggError, SimulationHandler, _ffi
from egg_fluid_simulation_amd.simulation_handler import Impulse

inf, nan = float("inf"), float("nan")

# ---------------------------------------------------------------------------- input -> records (a list) or the error text (a str)
# a record of a tagged kind list reads (kind, type_mask, p[0], p[1], ...)
COLLIDERS = [
    ([], []),
    ([('disc', 1, 2.5, -3)], [(1, 3, 1.0, 2.5, -3.0, 0.0)]),
    ([['disc', 1, 2.5, -3]], [(1, 3, 1.0, 2.5, -3.0, 0.0)]),
    ([{'cx': 1, 'cy': 2.5, 'R': -3, 'kind': 'disc'}], [(1, 3, 1.0, 2.5, -3.0, 0.0)]),
    ([('disc', 1, 2.5, -3, 'yolk')], [(1, 2, 1.0, 2.5, -3.0, 0.0)]),
    ([('segment', 1, 2, 3, 4, 'white'), ('disc', 1, 2.5, -3, 'both')], [(3, 1, 1.0, 2.0, 3.0, 4.0), (1, 3, 1.0, 2.5, -3.0, 0.0)]),
    ([{'x0': 1, 'y0': 2, 'x1': 3, 'y1': 4, 'kind': 'segment', 'types': 'white'}], [(3, 1, 1.0, 2.0, 3.0, 4.0)]),
    ([{'cx': 1, 'cy': 2.5, 'R': -3, 'kind': 'disc', 'types': 'yolk'}, ('disc', '1', True, -3)], [(1, 2, 1.0, 2.5, -3.0, 0.0), (1, 3, 1.0, 1.0, -3.0, 0.0)]),
    ([('blob', 1, 2.5, -3)], "collider 0: kind must be one of half_plane, disc, container, segment, wall, not 'blob'"),
    ([(3, 1, 2.5, -3)], 'collider 0: kind must be one of half_plane, disc, container, segment, wall, not 3'),
    ([(None, 1, 2.5, -3)], 'collider 0: kind must be one of half_plane, disc, container, segment, wall, not None'),
    ([()], 'collider 0: kind must be one of half_plane, disc, container, segment, wall, not None'),
    ([{'types': 'both'}], 'collider 0: kind must be one of half_plane, disc, container, segment, wall, not None'),
    ([{'kind': ['disc']}], "collider 0: kind must be one of half_plane, disc, container, segment, wall, not ['disc']"),
    ([('disc', 1, 2.5, -3), ('blob',)], "collider 1: kind must be one of half_plane, disc, container, segment, wall, not 'blob'"),
    ([{'cx': 1, 'cy': 2.5, 'kind': 'disc'}], 'collider 0 (disc): expected the keys cx, cy, R'),
    ([{'cx': 1, 'cy': 2.5, 'R': -3, 'kind': 'disc', 'z': 4}], 'collider 0 (disc): expected the keys cx, cy, R'),
    ([{'cx': 1, 'cy': 2.5, 'R': -3, 'kind': 'disc', 'z': 4, 'types': 'green'}], 'collider 0 (disc): expected the keys cx, cy, R'),
    ([('disc', 1, 2.5)], "collider 0 (disc): expected ('disc', cx, cy, R[, types])"),
    ([('disc',)], "collider 0 (disc): expected ('disc', cx, cy, R[, types])"),
    ([('disc', 1, 2.5, -3, 4)], "collider 0 (disc): expected ('disc', cx, cy, R[, types])"),
    ([('disc', 1, 2.5, -3, 4, 'yolk')], "collider 0 (disc): expected ('disc', cx, cy, R[, types])"),
    ([('disc', 1, 2.5, -3, 'green')], "collider 0: types must be 'both', 'white' or 'yolk', not 'green'"),
    ([('disc', 1, 2.5, -3, '')], "collider 0: types must be 'both', 'white' or 'yolk', not ''"),
    ([{'cx': 1, 'cy': 2.5, 'R': -3, 'kind': 'disc', 'types': 3}], "collider 0: types must be 'both', 'white' or 'yolk', not 3"),
    ([{'cx': 1, 'cy': 2.5, 'R': -3, 'kind': 'disc', 'types': None}], "collider 0: types must be 'both', 'white' or 'yolk', not None"),
    ([('disc', 1, 'x', -3)], 'collider 0 (disc): the parameters must be numbers'),
    ([('disc', 1, None, -3)], 'collider 0 (disc): the parameters must be numbers'),
    ([{'cx': 'x', 'cy': 2.5, 'R': -3, 'kind': 'disc'}], 'collider 0 (disc): the parameters must be numbers'),
    ([('disc', 1, 'x', -3, 'green')], "collider 0: types must be 'both', 'white' or 'yolk', not 'green'"),
    ([('disc', 1, 2.5, 'yolk')], 'collider 0 (disc): the parameters must be numbers'),
    ([('disc', 1, 'yolk')], "collider 0 (disc): expected ('disc', cx, cy, R[, types])"),
    ([('disc', 'yolk')], "collider 0 (disc): expected ('disc', cx, cy, R[, types])"),
    ([('disc', 1, 2.5, -3, 'yolk', 'white')], "collider 0 (disc): expected ('disc', cx, cy, R[, types])"),
    ([('wall', 1, 2, 3, 4), ('container', 5, 6, 7, 'white'), ('half_plane', 0, 2, 5)], [(5, 3, 1.0, 2.0, 3.0, 4.0), (2, 1, 5.0, 6.0, 7.0, 0.0), (0, 3, 0.0, 2.0, 5.0, 0.0)]),
    ([('box', 1, 2, 3, 4, 0.5)], "collider 0: kind must be one of half_plane, disc, container, segment, wall, not 'box'"),
    ([('disc', nan, inf, -1)], [(1, 3, nan, inf, -1.0, 0.0)]),
]

SENSORS = [
    ([], []),
    ([('disc', 1, 2.5, -3)], [(1, 3, 1.0, 2.5, -3.0, 0.0, 0.0, 0.0)]),
    ([['disc', 1, 2.5, -3]], [(1, 3, 1.0, 2.5, -3.0, 0.0, 0.0, 0.0)]),
    ([{'cx': 1, 'cy': 2.5, 'R': -3, 'kind': 'disc'}], [(1, 3, 1.0, 2.5, -3.0, 0.0, 0.0, 0.0)]),
    ([('disc', 1, 2.5, -3, 'yolk')], [(1, 2, 1.0, 2.5, -3.0, 0.0, 0.0, 0.0)]),
    ([('capsule', 1, 2, 3, 4, 5, 'white'), ('disc', 1, 2.5, -3, 'both')], [(3, 1, 1.0, 2.0, 3.0, 4.0, 5.0, 0.0), (1, 3, 1.0, 2.5, -3.0, 0.0, 0.0, 0.0)]),
    ([{'x0': 1, 'y0': 2, 'x1': 3, 'y1': 4, 'R': 5, 'kind': 'capsule', 'types': 'white'}], [(3, 1, 1.0, 2.0, 3.0, 4.0, 5.0, 0.0)]),
    ([{'cx': 1, 'cy': 2.5, 'R': -3, 'kind': 'disc', 'types': 'yolk'}, ('disc', '1', True, -3)], [(1, 2, 1.0, 2.5, -3.0, 0.0, 0.0, 0.0), (1, 3, 1.0, 1.0, -3.0, 0.0, 0.0, 0.0)]),
    ([('blob', 1, 2.5, -3)], "sensor 0: kind must be one of half_plane, disc, box, capsule, not 'blob'"),
    ([(3, 1, 2.5, -3)], 'sensor 0: kind must be one of half_plane, disc, box, capsule, not 3'),
    ([(None, 1, 2.5, -3)], 'sensor 0: kind must be one of half_plane, disc, box, capsule, not None'),
    ([()], 'sensor 0: kind must be one of half_plane, disc, box, capsule, not None'),
    ([{'types': 'both'}], 'sensor 0: kind must be one of half_plane, disc, box, capsule, not None'),
    ([{'kind': ['disc']}], "sensor 0: kind must be one of half_plane, disc, box, capsule, not ['disc']"),
    ([('disc', 1, 2.5, -3), ('blob',)], "sensor 1: kind must be one of half_plane, disc, box, capsule, not 'blob'"),
    ([{'cx': 1, 'cy': 2.5, 'kind': 'disc'}], 'sensor 0 (disc): expected the keys cx, cy, R'),
    ([{'cx': 1, 'cy': 2.5, 'R': -3, 'kind': 'disc', 'z': 4}], 'sensor 0 (disc): expected the keys cx, cy, R'),
    ([{'cx': 1, 'cy': 2.5, 'R': -3, 'kind': 'disc', 'z': 4, 'types': 'green'}], 'sensor 0 (disc): expected the keys cx, cy, R'),
    ([('disc', 1, 2.5)], "sensor 0 (disc): expected ('disc', cx, cy, R[, types])"),
    ([('disc',)], "sensor 0 (disc): expected ('disc', cx, cy, R[, types])"),
    ([('disc', 1, 2.5, -3, 4)], "sensor 0 (disc): expected ('disc', cx, cy, R[, types])"),
    ([('disc', 1, 2.5, -3, 4, 'yolk')], "sensor 0 (disc): expected ('disc', cx, cy, R[, types])"),
    ([('disc', 1, 2.5, -3, 'green')], "sensor 0: types must be 'both', 'white' or 'yolk', not 'green'"),
    ([('disc', 1, 2.5, -3, '')], "sensor 0: types must be 'both', 'white' or 'yolk', not ''"),
    ([{'cx': 1, 'cy': 2.5, 'R': -3, 'kind': 'disc', 'types': 3}], "sensor 0: types must be 'both', 'white' or 'yolk', not 3"),
    ([{'cx': 1, 'cy': 2.5, 'R': -3, 'kind': 'disc', 'types': None}], "sensor 0: types must be 'both', 'white' or 'yolk', not None"),
    ([('disc', 1, 'x', -3)], 'sensor 0 (disc): the parameters must be numbers'),
    ([('disc', 1, None, -3)], 'sensor 0 (disc): the parameters must be numbers'),
    ([{'cx': 'x', 'cy': 2.5, 'R': -3, 'kind': 'disc'}], 'sensor 0 (disc): the parameters must be numbers'),
    ([('disc', 1, 'x', -3, 'green')], "sensor 0: types must be 'both', 'white' or 'yolk', not 'green'"),
    ([('disc', 1, 2.5, 'yolk')], "sensor 0 (disc): expected ('disc', cx, cy, R[, types])"),
    ([('disc', 1, 'yolk')], "sensor 0 (disc): expected ('disc', cx, cy, R[, types])"),
    ([('disc', 'yolk')], "sensor 0 (disc): expected ('disc', cx, cy, R[, types])"),
    ([('disc', 1, 2.5, -3, 'yolk', 'white')], "sensor 0 (disc): expected ('disc', cx, cy, R[, types])"),
    ([('capsule', 1, 2, 3, 4, 5), {'kind': 'capsule', 'x0': 1, 'y0': 2, 'x1': 3, 'y1': 4, 'R': 5, 'types': 'white'}], [(3, 3, 1.0, 2.0, 3.0, 4.0, 5.0, 0.0), (3, 1, 1.0, 2.0, 3.0, 4.0, 5.0, 0.0)]),
    ([('half_plane', 0, 1, 2)] * 64, [(0, 3, 0.0, 1.0, 2.0, 0.0, 0.0, 0.0)] * 64),
    ([('half_plane', 0, 1, 2)] * 65, 'sensors: a list holds 0 .. 64 sensors, not 65'),
    ([('box', 1, 2, 3, 4, 0.0)], [(2, 3, 1.0, 2.0, 3.0, 4.0, 1.0, 0.0)]),
    ([('box', 1, 2, 3, 4, 0.25, 'yolk')], [(2, 2, 1.0, 2.0, 3.0, 4.0, 0.9689124217106447, 0.24740395925452294)]),
    ([{'kind': 'box', 'cx': 1, 'cy': 2, 'hx': 3, 'hy': 4, 'angle': 0.25}], [(2, 3, 1.0, 2.0, 3.0, 4.0, 0.9689124217106447, 0.24740395925452294)]),
    ([{'kind': 'box', 'cx': 1, 'cy': 2, 'hx': 3, 'hy': 4, 'angle': 0.25, 'types': 'white'}], [(2, 1, 1.0, 2.0, 3.0, 4.0, 0.9689124217106447, 0.24740395925452294)]),
    ([('box', 1, 2, 3, 4, 0.6, 0.8)], [(2, 3, 1.0, 2.0, 3.0, 4.0, 0.6, 0.8)]),
    ([('box', 1, 2, 3, 4, 0.6, 0.8, 'yolk')], [(2, 2, 1.0, 2.0, 3.0, 4.0, 0.6, 0.8)]),
    ([{'kind': 'box', 'cx': 1, 'cy': 2, 'hx': 3, 'hy': 4, 'ux': 0.6, 'uy': 0.8}], [(2, 3, 1.0, 2.0, 3.0, 4.0, 0.6, 0.8)]),
    ([{'kind': 'box', 'cx': 1, 'cy': 2, 'hx': 3, 'hy': 4, 'ux': 0.6, 'uy': 0.8, 'angle': 0.25}], 'sensor 0 (box): expected the keys cx, cy, hx, hy, ux, uy'),
    ([{'kind': 'box', 'cx': 1, 'cy': 2, 'hx': 3, 'hy': 4}], 'sensor 0 (box): expected the keys cx, cy, hx, hy, ux, uy'),
    ([('box', 1, 2, 3, 4)], "sensor 0 (box): expected ('box', cx, cy, hx, hy, ux, uy[, types])"),
    ([('box', 1, 2, 3, 4, 5, 6, 7)], "sensor 0 (box): expected ('box', cx, cy, hx, hy, ux, uy[, types])"),
    ([('box', 1, 2, 3, 4, 'x')], "sensor 0 (box): expected ('box', cx, cy, hx, hy, ux, uy[, types])"),
    ([('box', 1, 2, 3, 4, None)], 'sensor 0 (box): the parameters must be numbers'),
    ([{'kind': 'box', 'cx': 1, 'cy': 2, 'hx': 3, 'hy': 4, 'angle': 'x'}], 'sensor 0 (box): the parameters must be numbers'),
    ([('disc', 1, 2, 3, 4)], "sensor 0 (disc): expected ('disc', cx, cy, R[, types])"),
]

FORCES = [
    ([], []),
    ([('uniform', 1, 2.5)], [(0, 3, 1.0, 2.5, 0.0, 0.0)]),
    ([['uniform', 1, 2.5]], [(0, 3, 1.0, 2.5, 0.0, 0.0)]),
    ([{'gx': 1, 'gy': 2.5, 'kind': 'uniform'}], [(0, 3, 1.0, 2.5, 0.0, 0.0)]),
    ([('uniform', 1, 2.5, 'yolk')], [(0, 2, 1.0, 2.5, 0.0, 0.0)]),
    ([('vortex', 1, 2, 3, 4, 'white'), ('uniform', 1, 2.5, 'both')], [(2, 1, 1.0, 2.0, 3.0, 4.0), (0, 3, 1.0, 2.5, 0.0, 0.0)]),
    ([{'cx': 1, 'cy': 2, 'strength': 3, 'R': 4, 'kind': 'vortex', 'types': 'white'}], [(2, 1, 1.0, 2.0, 3.0, 4.0)]),
    ([{'gx': 1, 'gy': 2.5, 'kind': 'uniform', 'types': 'yolk'}, ('uniform', '1', True)], [(0, 2, 1.0, 2.5, 0.0, 0.0), (0, 3, 1.0, 1.0, 0.0, 0.0)]),
    ([('blob', 1, 2.5)], "field 0: kind must be one of uniform, radial, vortex, not 'blob'"),
    ([(3, 1, 2.5)], 'field 0: kind must be one of uniform, radial, vortex, not 3'),
    ([(None, 1, 2.5)], 'field 0: kind must be one of uniform, radial, vortex, not None'),
    ([()], 'field 0: kind must be one of uniform, radial, vortex, not None'),
    ([{'types': 'both'}], 'field 0: kind must be one of uniform, radial, vortex, not None'),
    ([{'kind': ['uniform']}], "field 0: kind must be one of uniform, radial, vortex, not ['uniform']"),
    ([('uniform', 1, 2.5), ('blob',)], "field 1: kind must be one of uniform, radial, vortex, not 'blob'"),
    ([{'gx': 1, 'kind': 'uniform'}], 'field 0 (uniform): expected the keys gx, gy'),
    ([{'gx': 1, 'gy': 2.5, 'kind': 'uniform', 'z': 4}], 'field 0 (uniform): expected the keys gx, gy'),
    ([{'gx': 1, 'gy': 2.5, 'kind': 'uniform', 'z': 4, 'types': 'green'}], 'field 0 (uniform): expected the keys gx, gy'),
    ([('uniform', 1)], "field 0 (uniform): expected ('uniform', gx, gy[, types])"),
    ([('uniform',)], "field 0 (uniform): expected ('uniform', gx, gy[, types])"),
    ([('uniform', 1, 2.5, 4)], "field 0 (uniform): expected ('uniform', gx, gy[, types])"),
    ([('uniform', 1, 2.5, 4, 'yolk')], "field 0 (uniform): expected ('uniform', gx, gy[, types])"),
    ([('uniform', 1, 2.5, 'green')], "field 0: types must be 'both', 'white' or 'yolk', not 'green'"),
    ([('uniform', 1, 2.5, '')], "field 0: types must be 'both', 'white' or 'yolk', not ''"),
    ([{'gx': 1, 'gy': 2.5, 'kind': 'uniform', 'types': 3}], "field 0: types must be 'both', 'white' or 'yolk', not 3"),
    ([{'gx': 1, 'gy': 2.5, 'kind': 'uniform', 'types': None}], "field 0: types must be 'both', 'white' or 'yolk', not None"),
    ([('uniform', 1, 'x')], 'field 0 (uniform): the parameters must be numbers'),
    ([('uniform', 1, None)], 'field 0 (uniform): the parameters must be numbers'),
    ([{'gx': 'x', 'gy': 2.5, 'kind': 'uniform'}], 'field 0 (uniform): the parameters must be numbers'),
    ([('uniform', 1, 'x', 'green')], "field 0: types must be 'both', 'white' or 'yolk', not 'green'"),
    ([('uniform', 1, 'yolk')], 'field 0 (uniform): the parameters must be numbers'),
    ([('uniform', 'yolk')], "field 0 (uniform): expected ('uniform', gx, gy[, types])"),
    ([('uniform', 1, 2.5, 'yolk', 'white')], "field 0 (uniform): expected ('uniform', gx, gy[, types])"),
    ([('uniform', 0, 980), {'kind': 'vortex', 'cx': 1, 'cy': 2, 'strength': 3, 'R': 4, 'types': 'yolk'}, ('radial', 1, 2, -3, 4, 'white')], [(0, 3, 0.0, 980.0, 0.0, 0.0), (2, 2, 1.0, 2.0, 3.0, 4.0), (1, 1, 1.0, 2.0, -3.0, 4.0)]),
    ([('uniform', 0, 980, 'yolk')], [(0, 2, 0.0, 980.0, 0.0, 0.0)]),
    ([('uniform', 0)], "field 0 (uniform): expected ('uniform', gx, gy[, types])"),
    ([{'kind': 'uniform', 'gx': 0, 'gy': 1, 'R': 2}], 'field 0 (uniform): expected the keys gx, gy'),
]

SURFACES = [
    ([], []),
    ([None], [(0.0, 0.0, 0.0)]),
    ([0.5], [(0.5, 0.0, 0.0)]),
    ([3], [(3.0, 0.0, 0.0)]),
    ([True], [(1.0, 0.0, 0.0)]),
    ([(0.25, 3, -4)], [(0.25, 3.0, -4.0)]),
    ([[0.25, 3, -4]], [(0.25, 3.0, -4.0)]),
    ([None, 0.5, ('1', 2, 3)], [(0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (1.0, 2.0, 3.0)]),
    ([(nan, inf, -inf)], [(nan, inf, -inf)]),
    ([-1.0], [(-1.0, 0.0, 0.0)]),
    ([nan], [(nan, 0.0, 0.0)]),
    ([()], 'collider surface 0: expected None, a number mu or (mu, vx, vy), not ()'),
    ([(1,)], 'collider surface 0: expected None, a number mu or (mu, vx, vy), not (1.0,)'),
    ([(1, 2)], 'collider surface 0: expected None, a number mu or (mu, vx, vy), not (1.0, 2.0)'),
    ([(1, 2, 3, 4)], 'collider surface 0: expected None, a number mu or (mu, vx, vy), not (1.0, 2.0, 3.0, 4.0)'),
    ([None, (1, 2)], 'collider surface 1: expected None, a number mu or (mu, vx, vy), not (1.0, 2.0)'),
    (['abc'], "collider surface 0: expected None, a number mu or (mu, vx, vy), not 'abc'"),
    (['1'], 'collider surface 0: expected None, a number mu or (mu, vx, vy), not (1.0,)'),
    ([(1, 'x', 3)], "collider surface 0: expected None, a number mu or (mu, vx, vy), not (1, 'x', 3)"),
    ([(1, None, 3)], 'collider surface 0: expected None, a number mu or (mu, vx, vy), not (1, None, 3)'),
    ([1j], 'collider surface 0: expected None, a number mu or (mu, vx, vy), not 1j'),
    ([{}], 'collider surface 0: expected None, a number mu or (mu, vx, vy), not ()'),
    ([None, None, 1j], 'collider surface 2: expected None, a number mu or (mu, vx, vy), not 1j'),
]

MOTIONS = [
    ([], []),
    ([None], [(0.0, 0.0)]),
    ([(3, -4)], [(3.0, -4.0)]),
    ([[3, -4]], [(3.0, -4.0)]),
    ([None, (0.5, '0.25')], [(0.0, 0.0), (0.5, 0.25)]),
    ([(-0.0, 0.0)], [(-0.0, 0.0)]),
    ([()], 'collider motion 0: expected None or (vx, vy), not ()'),
    ([(1,)], 'collider motion 0: expected None or (vx, vy), not (1.0,)'),
    ([(1, 2, 3)], 'collider motion 0: expected None or (vx, vy), not (1.0, 2.0, 3.0)'),
    ([None, (1, 2, 3)], 'collider motion 1: expected None or (vx, vy), not (1.0, 2.0, 3.0)'),
    ([(nan, 1)], 'collider motion 0: the velocity (nan, 1.0) is not finite'),
    ([(1, nan)], 'collider motion 0: the velocity (1.0, nan) is not finite'),
    ([(inf, 1)], 'collider motion 0: the velocity (inf, 1.0) is not finite'),
    ([(1, -inf)], 'collider motion 0: the velocity (1.0, -inf) is not finite'),
    ([(nan, inf)], 'collider motion 0: the velocity (nan, inf) is not finite'),
    ([(nan, 1, 2)], 'collider motion 0: expected None or (vx, vy), not (nan, 1.0, 2.0)'),
    ([5], 'collider motion 0: expected None or (vx, vy), not 5'),
    ([2.5], 'collider motion 0: expected None or (vx, vy), not 2.5'),
    (['ab'], "collider motion 0: expected None or (vx, vy), not 'ab'"),
    (['12'], [(1.0, 2.0)]),
    ([(1, 'x')], "collider motion 0: expected None or (vx, vy), not (1, 'x')"),
    ([(1, None)], 'collider motion 0: expected None or (vx, vy), not (1, None)'),
    ([None, None, 5], 'collider motion 2: expected None or (vx, vy), not 5'),
]

SPINS = [
    ([], []),
    ([None], [(0.0, 0.0, 0.0)]),
    ([(3, -4, 2)], [(3.0, -4.0, 2.0)]),
    ([[3, -4, 2]], [(3.0, -4.0, 2.0)]),
    ([None, (0.5, 0.25, '-0.125')], [(0.0, 0.0, 0.0), (0.5, 0.25, -0.125)]),
    ([()], 'collider spin 0: expected None or (px, py, omega), not ()'),
    ([(1, 2)], 'collider spin 0: expected None or (px, py, omega), not (1.0, 2.0)'),
    ([(1, 2, 3, 4)], 'collider spin 0: expected None or (px, py, omega), not (1.0, 2.0, 3.0, 4.0)'),
    ([None, (1, 2)], 'collider spin 1: expected None or (px, py, omega), not (1.0, 2.0)'),
    ([(nan, 1, 2)], 'collider spin 0: the pivot (nan, 1.0) is not finite'),
    ([(1, inf, 2)], 'collider spin 0: the pivot (1.0, inf) is not finite'),
    ([(1, 2, nan)], 'collider spin 0: omega nan is not finite'),
    ([(1, 2, -inf)], 'collider spin 0: omega -inf is not finite'),
    ([(nan, 1, nan)], 'collider spin 0: the pivot (nan, 1.0) is not finite'),
    ([(1, nan, inf)], 'collider spin 0: the pivot (1.0, nan) is not finite'),
    ([(nan, inf, nan)], 'collider spin 0: the pivot (nan, inf) is not finite'),
    ([(nan, 1)], 'collider spin 0: expected None or (px, py, omega), not (nan, 1.0)'),
    ([7], 'collider spin 0: expected None or (px, py, omega), not 7'),
    (['abc'], "collider spin 0: expected None or (px, py, omega), not 'abc'"),
    (['123'], [(1.0, 2.0, 3.0)]),
    ([(1, 'x', 3)], "collider spin 0: expected None or (px, py, omega), not (1, 'x', 3)"),
    ([(1, 2, None)], 'collider spin 0: expected None or (px, py, omega), not (1, 2, None)'),
    ([None, None, 7], 'collider spin 2: expected None or (px, py, omega), not 7'),
]

BODIES = [
    ([], []),
    ([None], [(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)]),
    ([(0.5, 0.25)], [(0.5, 0.25, 0.0, 0.0, 0.0, 0.0)]),
    ([(0.5, 0.25, 3, -4)], [(0.5, 0.25, 3.0, -4.0, 0.0, 0.0)]),
    ([(0.5, 0.25, -3, 4, 0.125, 2)], [(0.5, 0.25, -3.0, 4.0, 0.125, 2.0)]),
    ([[0.5, 0.25]], [(0.5, 0.25, 0.0, 0.0, 0.0, 0.0)]),
    ([None, ('1', 0), (0, 0, -1, -2, 0, 0)], [(0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0, 0.0, 0.0), (0.0, 0.0, -1.0, -2.0, 0.0, 0.0)]),
    ([(-0.0, -0.0)], [(-0.0, -0.0, 0.0, 0.0, 0.0, 0.0)]),
    ([(0.0, 0.0, -0.0, -0.0, -0.0, -0.0)], [(0.0, 0.0, -0.0, -0.0, -0.0, -0.0)]),
    ([()], 'collider body 0: expected None or (inv_mass, inv_inertia[, ax, ay[, drag, spin_drag]]), not ()'),
    ([(1,)], 'collider body 0: expected None or (inv_mass, inv_inertia[, ax, ay[, drag, spin_drag]]), not (1.0,)'),
    ([(1, 2, 3)], 'collider body 0: expected None or (inv_mass, inv_inertia[, ax, ay[, drag, spin_drag]]), not (1.0, 2.0, 3.0)'),
    ([(1, 2, 3, 4, 5)], 'collider body 0: expected None or (inv_mass, inv_inertia[, ax, ay[, drag, spin_drag]]), not (1.0, 2.0, 3.0, 4.0, 5.0)'),
    ([(1, 2, 3, 4, 5, 6, 7)], 'collider body 0: expected None or (inv_mass, inv_inertia[, ax, ay[, drag, spin_drag]]), not (1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0)'),
    ([None, (1, 2, 3)], 'collider body 1: expected None or (inv_mass, inv_inertia[, ax, ay[, drag, spin_drag]]), not (1.0, 2.0, 3.0)'),
    ([(nan, 1)], 'collider body 0: inv_mass nan is not finite'),
    ([(1, nan)], 'collider body 0: inv_inertia nan is not finite'),
    ([(1, 1, nan, 0)], 'collider body 0: ax nan is not finite'),
    ([(1, 1, 0, nan)], 'collider body 0: ay nan is not finite'),
    ([(1, 1, 0, 0, nan, 0)], 'collider body 0: drag nan is not finite'),
    ([(1, 1, 0, 0, 0, nan)], 'collider body 0: spin_drag nan is not finite'),
    ([(inf, 1)], 'collider body 0: inv_mass inf is not finite'),
    ([(1, -inf)], 'collider body 0: inv_inertia -inf is not finite'),
    ([(1, 1, inf, 0)], 'collider body 0: ax inf is not finite'),
    ([(1, 1, 0, -inf)], 'collider body 0: ay -inf is not finite'),
    ([(1, 1, 0, 0, inf, 0)], 'collider body 0: drag inf is not finite'),
    ([(1, 1, 0, 0, 0, -inf)], 'collider body 0: spin_drag -inf is not finite'),
    ([(-1, 1)], 'collider body 0: inv_mass -1.0 is negative'),
    ([(1, -1)], 'collider body 0: inv_inertia -1.0 is negative'),
    ([(1, 1, 0, 0, -1, 0)], 'collider body 0: drag -1.0 is negative'),
    ([(1, 1, 0, 0, 0, -1)], 'collider body 0: spin_drag -1.0 is negative'),
    ([(1, 1, -5, -6)], [(1.0, 1.0, -5.0, -6.0, 0.0, 0.0)]),
    ([(-1, nan)], 'collider body 0: inv_mass -1.0 is negative'),
    ([(nan, -1)], 'collider body 0: inv_mass nan is not finite'),
    ([(1, 1, nan, 0, -1, 0)], 'collider body 0: ax nan is not finite'),
    ([(1, -1, nan, 0)], 'collider body 0: inv_inertia -1.0 is negative'),
    ([(1, 1, 0, 0, -1, nan)], 'collider body 0: drag -1.0 is negative'),
    ([(nan, 1, 2)], 'collider body 0: expected None or (inv_mass, inv_inertia[, ax, ay[, drag, spin_drag]]), not (nan, 1.0, 2.0)'),
    ([3], 'collider body 0: expected None or (inv_mass, inv_inertia[, ax, ay[, drag, spin_drag]]), not 3'),
    (['ab'], "collider body 0: expected None or (inv_mass, inv_inertia[, ax, ay[, drag, spin_drag]]), not 'ab'"),
    (['12'], [(1.0, 2.0, 0.0, 0.0, 0.0, 0.0)]),
    ([(1, 'x')], "collider body 0: expected None or (inv_mass, inv_inertia[, ax, ay[, drag, spin_drag]]), not (1, 'x')"),
    ([(1, None)], 'collider body 0: expected None or (inv_mass, inv_inertia[, ax, ay[, drag, spin_drag]]), not (1, None)'),
    ([None, None, 3], 'collider body 2: expected None or (inv_mass, inv_inertia[, ax, ay[, drag, spin_drag]]), not 3'),
]

PAIRS = [
    ((0, 1), (0.0, 1.0)),
    ((0.0, 0.0), (0.0, 0.0)),
    ((2.5, 0.5), (2.5, 0.5)),
    ((1, 1.0), (1.0, 1.0)),
    (('2', '0.5'), (2.0, 0.5)),
    ((True, False), (1.0, 0.0)),
    ((-0.0, 1), (-0.0, 1.0)),
    ((1, -0.0), (1.0, -0.0)),
    ((1e+308, 1), (1e+308, 1.0)),
    ((nan, 1), '%(what)s: the %(first)s nan is not a finite number >= 0'),
    ((inf, 1), '%(what)s: the %(first)s inf is not a finite number >= 0'),
    ((-inf, 1), '%(what)s: the %(first)s -inf is not a finite number >= 0'),
    ((-1, 1), '%(what)s: the %(first)s -1.0 is not a finite number >= 0'),
    ((-1e-300, 1), '%(what)s: the %(first)s -1e-300 is not a finite number >= 0'),
    (('x', 1), "%(what)s: the %(first)s must be a number, not 'x'"),
    ((None, 1), '%(what)s: the %(first)s must be a number, not None'),
    (([1], 1), '%(what)s: the %(first)s must be a number, not [1]'),
    ((1, 'x'), "%(what)s: the strength must be a number, not 'x'"),
    ((1, None), '%(what)s: the strength must be a number, not None'),
    (('x', 'y'), "%(what)s: the %(first)s must be a number, not 'x'"),
    ((1, 1.0000000000000002), '%(what)s: the strength 1.0000000000000002 lies outside [0, 1]'),
    ((1, 2), '%(what)s: the strength 2.0 lies outside [0, 1]'),
    ((1, nan), '%(what)s: the strength nan lies outside [0, 1]'),
    ((1, inf), '%(what)s: the strength inf lies outside [0, 1]'),
    ((1, -0.1), '%(what)s: the strength -0.1 lies outside [0, 1]'),
    ((1, -1e-300), '%(what)s: the strength -1e-300 lies outside [0, 1]'),
    ((nan, 2), '%(what)s: the %(first)s nan is not a finite number >= 0'),
    ((-1, 'x'), "%(what)s: the strength must be a number, not 'x'"),
    ((nan, nan), '%(what)s: the %(first)s nan is not a finite number >= 0'),
]

IMPULSES = [
    ([], []),
    ([('kick', ('disc', 1, 2, 3), 4, 5)], [(0, 0, -1, 4.0, 5.0, 0.0, 1, 3, 1.0, 2.0, 3.0, 0.0, 0.0, 0.0)]),
    ([Impulse('blast', ('box', 1, 2, 3, 4, 0.0, 'yolk'), (1, 2, -4), 7, True, True), ('brake', {'kind': 'capsule', 'x0': 1, 'y0': 2, 'x1': 3, 'y1': 4, 'R': 5}, 0, 0, 1, {'linear': True})], [(1, 3, 7, 1.0, 2.0, -4.0, 2, 2, 1.0, 2.0, 3.0, 4.0, 1.0, 0.0), (3, 1, -1, 0.0, 0.0, 1.0, 3, 3, 1.0, 2.0, 3.0, 4.0, 5.0, 0.0)]),
    ([('kick', ('blob', 1, 2, 3), 4, 5)], "impulse: record 0: region: sensor 0: kind must be one of half_plane, disc, box, capsule, not 'blob'"),
    ([('kick', ('disc', 1, 2), 4, 5)], "impulse: record 0: region: sensor 0 (disc): expected ('disc', cx, cy, R[, types])"),
    ([('kick', ('disc', 1, 2, 'yolk'), 4, 5)], "impulse: record 0: region: sensor 0 (disc): expected ('disc', cx, cy, R[, types])"),
    ([('kick', ('disc', 1, 2, 3, 'green'), 4, 5)], "impulse: record 0: region: sensor 0: types must be 'both', 'white' or 'yolk', not 'green'"),
    ([('kick', ('disc', 1, 'x', 3), 4, 5)], 'impulse: record 0: region: sensor 0 (disc): the parameters must be numbers'),
    ([('kick', {'kind': 'disc', 'cx': 1, 'cy': 2}, 4, 5)], 'impulse: record 0: region: sensor 0 (disc): expected the keys cx, cy, R'),
    ([('kick', ('disc', 1, 2, 3), 4, 5), ('swirl', (), 1, 2, 3)], 'impulse: record 1: region: sensor 0: kind must be one of half_plane, disc, box, capsule, not None'),
    ([('kick', [('disc', 1, 2, 3), ('disc', 1, 2, 3)], 4, 5)], "impulse: record 0: region: sensor 0: kind must be one of half_plane, disc, box, capsule, not ('disc', 1, 2, 3)"),
    ([('kick', ('disc', 1, 2, 3), 4)], 'impulse: record 0 (kick): expected the parameters (ax, ay)'),
    ([('kick', ('disc', 1, 2), 4)], 'impulse: record 0 (kick): expected the parameters (ax, ay)'),
    ([('kick', ('disc', 1, 2), 'x', 5)], 'impulse: record 0 (kick): the parameters must be numbers'),
    ([('push', ('disc', 1, 2), 4, 5)], "impulse: record 0: action must be one of kick, blast, swirl, brake, not 'push'"),
]

MEASURE_SPECS = [
    ((None, 'both'), (0, 3, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)),
    ((('disc', 1, 2, 3, 'yolk'), 'white'), (1, 1, 1, 2, 1.0, 2.0, 3.0, 0.0, 0.0, 0.0)),
    (({'kind': 'box', 'cx': 1, 'cy': 2, 'hx': 3, 'hy': 4, 'angle': 0.0}, 2), (1, 2, 2, 3, 1.0, 2.0, 3.0, 4.0, 1.0, 0.0)),
    ((('blob', 1, 2, 3), 'both'), "measure: region: sensor 0: kind must be one of half_plane, disc, box, capsule, not 'blob'"),
    ((('disc', 1, 2), 'both'), "measure: region: sensor 0 (disc): expected ('disc', cx, cy, R[, types])"),
    ((('disc', 1, 2, 'yolk'), 3), "measure: region: sensor 0 (disc): expected ('disc', cx, cy, R[, types])"),
    ((('disc', 1, 2, 3), 'green'), "measure: types must be 'both', 'white', 'yolk' or a mask 1 .. 3, not 'green'"),
]


def _kinds(helper):
    def read(items):
        n, arr = helper(items)
        return [(arr[k].kind, arr[k].type_mask) + tuple(arr[k].p) for k in range(n)]
    return read


def _records(helper, fields):
    def read(items):
        n, arr = helper(items)
        return [tuple(getattr(arr[k], f) for f in fields) for k in range(n)]
    return read


def _impulses(items):
    n, arr = SimulationHandler._c_impulses(items)
    return [(arr[k].action, arr[k].flags, arr[k].id) + tuple(arr[k].a) + (arr[k].region.kind, arr[k].region.type_mask) + tuple(arr[k].region.p)
            for k in range(n)]


def _measure_spec(args):
    s = SimulationHandler._c_measure_spec(*args)
    return (s.flags, s.type_mask, s.region.kind, s.region.type_mask) + tuple(s.region.p)


def _pairs(helper, what, first):
    return [(lambda args: helper(*args), args, want % dict(what=what, first=first) if isinstance(want, str) else want) for args, want in PAIRS]


def _cases():
    tables = [("colliders", _kinds(SimulationHandler._c_colliders), COLLIDERS), ("sensors", _kinds(SimulationHandler._c_sensors), SENSORS),
              ("forces", _kinds(SimulationHandler._c_forces), FORCES),
              ("surfaces", _records(SimulationHandler._c_surfaces, ("friction", "vx", "vy")), SURFACES),
              ("motions", _records(SimulationHandler._c_motions, ("vx", "vy")), MOTIONS),
              ("spins", _records(SimulationHandler._c_spins, ("px", "py", "omega")), SPINS),
              ("bodies", _records(SimulationHandler._c_bodies, ("inv_mass", "inv_inertia", "ax", "ay", "drag", "spin_drag")), BODIES),
              ("impulses", _impulses, IMPULSES), ("measure_spec", _measure_spec, MEASURE_SPECS)]
    out = [(name, read, given, want) for name, read, table in tables for given, want in table]
    for name, helper, first in (("coupling", SimulationHandler._c_coupling, "factor"), ("adhesion", SimulationHandler._c_adhesion, "reach"),
                                ("containment", SimulationHandler._c_containment, "factor")):
        out += [(name, read, given, want) for read, given, want in _pairs(helper, name, first)]
    return out


@pytest.mark.parametrize("name", ["colliders", "sensors", "forces", "surfaces", "motions", "spins", "bodies", "impulses", "measure_spec",
                                  "coupling", "adhesion", "containment"])
def test_every_case_of_a_helper(name):
    cases = [c for c in _cases() if c[0] == name]
    assert len(cases) >= 7
    for _, read, given, want in cases:
        if isinstance(want, str):
            with pytest.raises(EggError) as e:
                read(given)
            assert str(e.value) == want, (given, str(e.value))
        else:
            got = read(given)
            assert repr(got) == repr(want), (given, got)


# ---------------------------------------------------------------------------- struct arrays filled by hand -> what the getters return
class _Stored(SimulationHandler):
    """a handler without a device whose entry points answer from `stored`: name -> a list of records (array getters), a
    tuple of doubles (pair getters) or integers (counter getters)"""

    def __init__(self, stored):
        self.stored, self.asked = stored, []

    def __del__(self):
        pass

    def _c(self, name):
        def call(*args):
            self.asked.append(name)
            value = self.stored[name]
            if isinstance(value, list):      # (..., cap, arr, &n)
                arr, n = args[-2], args[-1]._obj
                assert args[-3] >= len(value)
                for k, rec in enumerate(value):
                    arr[k] = rec
                n.value = len(value)
            elif len(args) == 1 and isinstance(args[0], C.Array):  # (int64[2])
                args[0][:] = value
            else:                            # (&a[, &b])
                for ref, v in zip(args, value):
                    ref._obj.value = v
            return _ffi.EGG_OK
        return call


def _kind_record(struct, kind, mask, *p):
    rec = struct(kind, mask)
    rec.p[:len(p)] = p
    return rec


def test_the_getters_decode_a_stored_array():
    h = _Stored({
        "get_colliders": [_kind_record(_ffi.EggCollider, 0, 3, 0.0, 1.0, 5.0, 9.0), _kind_record(_ffi.EggCollider, 1, 1, 1.0, 2.0, 3.0, 9.0),
                          _kind_record(_ffi.EggCollider, 2, 2, 4.0, 5.0, 6.0, 9.0), _kind_record(_ffi.EggCollider, 3, 3, 1.0, 2.0, 3.0, 4.0),
                          _kind_record(_ffi.EggCollider, 5, 2, 5.0, 6.0, 7.0, 8.0)],
        "get_collider_pose": [_kind_record(_ffi.EggCollider, 5, 1, 0.5, 1.5, 2.5, 3.5), _kind_record(_ffi.EggCollider, 1, 3, -1.0, -2.0, 3.0, 9.0)],
        "get_sensors": [_kind_record(_ffi.EggSensor, 0, 3, 0.0, 1.0, 2.0, 9.0, 9.0, 9.0), _kind_record(_ffi.EggSensor, 1, 2, 1.0, 2.0, 3.0, 9.0, 9.0, 9.0),
                        _kind_record(_ffi.EggSensor, 2, 1, 1.0, 2.0, 3.0, 4.0, 0.6, 0.8), _kind_record(_ffi.EggSensor, 3, 3, 1.0, 2.0, 3.0, 4.0, 5.0, 9.0)],
        "get_forces": [_kind_record(_ffi.EggForce, 0, 3, 0.0, 980.0, 9.0, 9.0), _kind_record(_ffi.EggForce, 1, 1, 1.0, 2.0, -3.0, 4.0),
                       _kind_record(_ffi.EggForce, 2, 2, 1.0, 2.0, 3.0, 4.0)],
        "get_collider_surfaces": [_ffi.EggColliderSurface(0.5, 3.0, -4.0), _ffi.EggColliderSurface()],
        "get_collider_motion": [_ffi.EggColliderMotion(3.0, -4.0), _ffi.EggColliderMotion()],
        "get_collider_spin": [_ffi.EggColliderSpin(1.0, 2.0, -0.5), _ffi.EggColliderSpin()],
        "get_collider_bodies": [_ffi.EggColliderBody(0.5, 0.25, 3.0, -4.0, 0.125, 2.0), _ffi.EggColliderBody()],
        "get_collider_loads": [_ffi.EggColliderLoad(1.5, -2.5, 0.75), _ffi.EggColliderLoad()],
    })
    assert h.get_colliders() == [("half_plane", 0.0, 1.0, 5.0, "both"), ("disc", 1.0, 2.0, 3.0, "white"), ("container", 4.0, 5.0, 6.0, "yolk"),
                                 ("segment", 1.0, 2.0, 3.0, 4.0, "both"), ("wall", 5.0, 6.0, 7.0, 8.0, "yolk")]
    assert h.get_collider_pose(0.25) == [("wall", 0.5, 1.5, 2.5, 3.5, "white"), ("disc", -1.0, -2.0, 3.0, "both")]
    assert h.get_sensors() == [("half_plane", 0.0, 1.0, 2.0, "both"), ("disc", 1.0, 2.0, 3.0, "yolk"), ("box", 1.0, 2.0, 3.0, 4.0, 0.6, 0.8, "white"),
                               ("capsule", 1.0, 2.0, 3.0, 4.0, 5.0, "both")]
    assert h.get_forces() == [("uniform", 0.0, 980.0, "both"), ("radial", 1.0, 2.0, -3.0, 4.0, "white"), ("vortex", 1.0, 2.0, 3.0, 4.0, "yolk")]
    assert h.get_collider_surfaces() == [(0.5, 3.0, -4.0), (0.0, 0.0, 0.0)]
    assert h.get_collider_motion() == [(3.0, -4.0), (0.0, 0.0)]
    assert h.get_collider_spin() == [(1.0, 2.0, -0.5), (0.0, 0.0, 0.0)]
    assert h.get_collider_bodies() == [(0.5, 0.25, 3.0, -4.0, 0.125, 2.0), (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)]
    assert h.collider_loads() == [(1.5, -2.5, 0.75), (0.0, 0.0, 0.0)]
    assert h.asked == ["get_colliders", "get_collider_pose", "get_sensors", "get_forces", "get_collider_surfaces", "get_collider_motion",
                       "get_collider_spin", "get_collider_bodies", "get_collider_loads"]
    for getter in (h.get_colliders, h.get_sensors, h.get_forces, h.get_collider_surfaces, h.get_collider_bodies):
        assert all(type(rec) is tuple for rec in getter())
    h.stored = {name: [] for name in h.stored}
    assert h.get_colliders() == h.get_sensors() == h.get_forces() == h.get_collider_surfaces() == h.get_collider_pose() == []


def test_the_getters_of_two_doubles_and_of_counters():
    h = _Stored({"get_coupling": (1.5, 0.25), "get_adhesion": (2.5, 0.5), "get_containment": (3.0, 0.75),
                 "get_coupling_solves": (11,), "get_adhesion_solves": (12,), "get_containment_hits": (13,), "get_collider_contact_solves": (1 << 40,),
                 "get_collider_hits": (3, 1 << 40), "get_collider_grips": (5, 6), "get_viscosity_pairs": (7, 8)})
    assert (h.coupling(), h.adhesion(), h.containment()) == ((1.5, 0.25), (2.5, 0.5), (3.0, 0.75))
    counters = (h.coupling_solves(), h.adhesion_solves(), h.containment_hits(), h.collider_contact_solves())
    assert counters == (11, 12, 13, 1 << 40) and all(type(v) is int for v in counters)
    assert (h.collider_hits(), h.collider_grips(), h.viscosity_pairs()) == ([3, 1 << 40], [5, 6], [7, 8])
    assert h.asked == ["get_coupling", "get_adhesion", "get_containment", "get_coupling_solves", "get_adhesion_solves", "get_containment_hits",
                       "get_collider_contact_solves", "get_collider_hits", "get_collider_grips", "get_viscosity_pairs"]


def test_the_timing_script_runs_without_a_device():
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "host_marshalling_bench.py"), "--repeat", "1", "--number", "2"],
                         check=True, capture_output=True, text=True, timeout=120).stdout
    rows = [json.loads(line) for line in out.splitlines()]
    assert [r["helper"] for r in rows] == ["_c_probes/1", "_c_sensors/1", "_c_impulses/1", "_c_probes/16", "_c_sensors/16", "_c_impulses/16",
                                           "_c_field_spec", "_c_measure_spec", "_c_measure_spec/region"]
    assert all(0.0 < r["min_us"] <= r["median_us"] <= r["max_us"] and (r["repeat"], r["number"]) == (1, 2) for r in rows)
