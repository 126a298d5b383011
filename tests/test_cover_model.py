"""The numpy model of the cover (tests/cover_model.py; include/eggsim_cover.h) against a hand table with the expected planes
written out, the rectangle the kernel tests against the every-cell definition on random small grids, and the refusal of a
grid that does not resolve its coordinates.  tests/test_gpu_cover.py runs the same table on the device."""
import numpy as np
import pytest

import cover_model as cm

# the hand table: per case the grid (x0, y0, cell, nx, ny), the scale, the types and per batch (id 1, 2, ...) the white and
# the yolk particles as (x, y, radius)
NAN, INF = float("nan"), float("inf")
FAR = (-1000.0, -1000.0, 1.0)
CASES = {
    "tangent_3_4_5": dict(grid=(0.0, 0.0, 1.0, 10, 10), scale=1.0, types="both",
                          batches=[([(1.5, 1.5, 5.0)], [(1.5, 1.5, float(np.nextafter(5.0, 0.0)))])]),
    "zero_radius": dict(grid=(0.0, 0.0, 1.0, 4, 4), scale=1.0, types="both",
                        batches=[([(1.5, 2.5, 0.0), (2.25, 0.5, 0.0)], [(0.5, 0.5, 0.0)])]),
    "span_limit": dict(grid=(0.0, 0.0, 1.0, 4, 4), scale=1.0, types="both",
                       batches=[([(2.0, 2.0, 64.0), (2.0, 2.0, float(np.nextafter(64.0, INF)))], [FAR])]),
    "span_limit_scaled": dict(grid=(0.0, 0.0, 0.5, 4, 4), scale=8.0, types="both",
                              batches=[([(1.0, 1.0, 4.0)], [(1.0, 1.0, float(np.nextafter(4.0, INF)))])]),
    "bad_values": dict(grid=(0.0, 0.0, 1.0, 4, 4), scale=1.0, types="both",
                       batches=[([(1.5, 1.5, -1.0), (1.5, 1.5, NAN), (NAN, 1.5, 1.0), (1.5, INF, 1.0), (-INF, 1.5, 1.0), (1.5, 1.5, 1.0)],
                                 [(1.5, 1.5, INF), (2.5, 2.5, 0.5)])]),
    "larger_than_grid": dict(grid=(-2.5, -1.5, 1.0, 5, 3), scale=1.0, types="both", batches=[([(0.0, 0.0, 50.0)], [(0.0, 0.0, 3.0)])]),
    "edges_and_corners": dict(grid=(10.0, 20.0, 2.0, 6, 5), scale=1.0, types="both",
                              batches=[([(10.0, 25.0, 2.5), (22.0, 25.0, 2.5), (16.0, 20.0, 2.5), (16.0, 30.0, 2.5)],
                                        [(10.0, 20.0, 3.0), (22.0, 20.0, 3.0), (10.0, 30.0, 3.0), (22.0, 30.0, 3.0)])]),
    "touch_no_centre": dict(grid=(0.0, 0.0, 1.0, 4, 4), scale=1.0, types="both",
                            batches=[([(-0.3, 2.0, 0.4), (1.0, 1.0, 0.3), (4.2, 4.2, 0.25)], [(2.0, -0.4, 0.45), (-0.5, 1.0, 0.4)])]),
    "owner_two": dict(grid=(0.0, 0.0, 1.0, 6, 3), scale=1.0, types="both",
                      batches=[([(3.5, 1.5, 1.5)], [(3.5, 1.5, 0.5)]), ([(2.5, 1.5, 1.5)], [(3.5, 1.5, 1.0)])]),
    "owner_three": dict(grid=(0.0, 0.0, 1.0, 7, 3), scale=1.0, types="both",
                        batches=[([(4.5, 1.5, 1.0)], [FAR]), ([(3.5, 1.5, 2.0)], [(3.5, 1.5, 1.0)]), ([(2.5, 1.5, 1.0)], [(2.5, 1.5, 1.0)])]),
    "white_only": dict(grid=(0.0, 0.0, 1.0, 4, 4), scale=1.0, types="white", batches=[([(1.5, 1.5, 1.0)], [(2.5, 2.5, 1.0)])]),
    "yolk_only": dict(grid=(0.0, 0.0, 1.0, 4, 4), scale=1.0, types="yolk", batches=[([(1.5, 1.5, 1.0)], [(2.5, 2.5, 1.0)])]),
    "scale_12": dict(grid=(0.5, 0.25, 1.5, 6, 4), scale=12.0, types="both", batches=[([(5.0, 3.25, 0.25)], [(2.75, 1.0, 0.125)])]),
}


def arrays(case):
    out = [[[], [], [], []], [[], [], [], []]]
    for k, b in enumerate(case["batches"]):
        for w in (0, 1):
            for (x, y, r) in b[w]:
                out[w][0].append(x); out[w][1].append(y); out[w][2].append(r); out[w][3].append(k + 1)
    return [[np.array(out[w][f], dtype=np.float64) for w in (0, 1)] for f in range(4)]

# what the rule gives, written out: rows of the planes from iy = 0 up, a digit per cell ("." in an owner plane: -1), then
# inside, outside, dropped, hits, covered per type, covered_both, covered_any
EXPECTED = {
    "tangent_3_4_5": dict(cover=(('1111110000', '1111111000', '1111110000', '1111110000', '1111110000', '1111100000', '0100000000', '0000000000', '0000000000', '0000000000'),
                  ('1111110000', '1111110000', '1111110000', '1111110000', '1111100000', '1111000000', '0000000000', '0000000000', '0000000000', '0000000000')),
         owner=(('111111....', '1111111...', '111111....', '111111....', '111111....', '11111.....', '.1........', '..........', '..........', '..........'),
                  ('111111....', '111111....', '111111....', '111111....', '11111.....', '1111......', '..........', '..........', '..........', '..........')),
         totals=((1, 1), (0, 0), (0, 0), (37, 33), (37, 33), 33, 37)),
    "zero_radius": dict(cover=(('0000', '0000', '0100', '0000'),
                  ('1000', '0000', '0000', '0000')),
         owner=(('....', '....', '.1..', '....'),
                  ('1...', '....', '....', '....')),
         totals=((2, 1), (0, 0), (0, 0), (1, 1), (1, 1), 0, 2)),
    "span_limit": dict(cover=(('1111', '1111', '1111', '1111'),
                  ('0000', '0000', '0000', '0000')),
         owner=(('1111', '1111', '1111', '1111'),
                  ('....', '....', '....', '....')),
         totals=((1, 0), (0, 1), (1, 0), (16, 0), (16, 0), 0, 16)),
    "span_limit_scaled": dict(cover=(('1111', '1111', '1111', '1111'),
                  ('0000', '0000', '0000', '0000')),
         owner=(('1111', '1111', '1111', '1111'),
                  ('....', '....', '....', '....')),
         totals=((1, 0), (0, 0), (0, 1), (16, 0), (16, 0), 0, 16)),
    "bad_values": dict(cover=(('0100', '1110', '0100', '0000'),
                  ('0000', '0000', '0010', '0000')),
         owner=(('.1..', '111.', '.1..', '....'),
                  ('....', '....', '..1.', '....')),
         totals=((1, 1), (0, 0), (5, 1), (5, 1), (5, 1), 0, 6)),
    "larger_than_grid": dict(cover=(('11111', '11111', '11111'),
                  ('11111', '11111', '11111')),
         owner=(('11111', '11111', '11111'),
                  ('11111', '11111', '11111')),
         totals=((1, 1), (0, 0), (0, 0), (15, 15), (15, 15), 15, 15)),
    "edges_and_corners": dict(cover=(('001100', '100001', '100001', '100001', '001100'),
                  ('100001', '000000', '000000', '000000', '100001')),
         owner=(('..11..', '1....1', '1....1', '1....1', '..11..'),
                  ('1....1', '......', '......', '......', '1....1')),
         totals=((4, 4), (0, 0), (0, 0), (10, 4), (10, 4), 0, 14)),
    "touch_no_centre": dict(cover=(('0000', '0000', '0000', '0000'),
                  ('0000', '0000', '0000', '0000')),
         owner=(('....', '....', '....', '....'),
                  ('....', '....', '....', '....')),
         totals=((3, 1), (0, 1), (0, 0), (0, 0), (0, 0), 0, 0)),
    "owner_two": dict(cover=(('012210', '012210', '012210'),
                  ('000100', '001210', '000100')),
         owner=(('.2111.', '.2111.', '.2111.'),
                  ('...2..', '..212.', '...2..')),
         totals=((2, 2), (0, 0), (0, 0), (18, 6), (12, 5), 5, 12)),
    "owner_three": dict(cover=(('0021200', '0223220', '0021200'),
                  ('0011000', '0122100', '0011000')),
         owner=(('..221..', '.22111.', '..221..'),
                  ('..32...', '.3222..', '..32...')),
         totals=((3, 2), (0, 1), (0, 0), (21, 10), (11, 8), 8, 11)),
    "white_only": dict(cover=(('0100', '1110', '0100', '0000'),
                  ('0000', '0000', '0000', '0000')),
         owner=(('.1..', '111.', '.1..', '....'),
                  ('....', '....', '....', '....')),
         totals=((1, 0), (0, 0), (0, 0), (5, 0), (5, 0), 0, 5)),
    "yolk_only": dict(cover=(('0000', '0000', '0000', '0000'),
                  ('0000', '0010', '0111', '0010')),
         owner=(('....', '....', '....', '....'),
                  ('....', '..1.', '.111', '..1.')),
         totals=((0, 1), (0, 0), (0, 0), (0, 5), (0, 5), 0, 5)),
    "scale_12": dict(cover=(('001100', '011110', '011110', '001100'),
                  ('111000', '010000', '000000', '000000')),
         owner=(('..11..', '.1111.', '.1111.', '..11..'),
                  ('111...', '.1....', '......', '......')),
         totals=((1, 1), (0, 0), (0, 0), (12, 4), (12, 4), 2, 14)),
}


def planes(rows, none):
    """a pair of tuples of row strings as an int32 array [2][ny][nx]: a digit is its value, '.' is `none`"""
    return np.array([[[none if c == "." else int(c, 36) for c in row] for row in p] for p in rows], dtype=np.int32)


def expected(name):
    e = EXPECTED[name]
    return (planes(e["cover"], 0), planes(e["owner"], -1)) + tuple(e["totals"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_case(name):
    case = CASES[name]
    x, y, r, b = arrays(case)
    for full in (False, True):
        got = cm.cover(case["grid"], case["scale"], x, y, r, b, case["types"], True, full)
        assert cm.same(got, expected(name)), (name, full, got)
    assert set(CASES) == set(EXPECTED)


def test_the_cells_the_table_is_about():
    """the cells the cases were built for, by their own arithmetic"""
    cover = expected("tangent_3_4_5")[0]
    assert (4.5 - 1.5) ** 2 + (5.5 - 1.5) ** 2 == 25.0 and cover[0][5][4] == 1 and cover[1][5][4] == 0  # dx = 3, dy = 4, R = 5 and just below
    assert cover[0][6][1] == 1 and cover[0][1][6] == 1 and cover[1][6][1] == 0 and cover[1][1][6] == 0      # the axis tangents
    assert expected("zero_radius")[5] == (1, 1) and expected("zero_radius")[2] == (2, 1)                     # on a centre: 1 hit, off: none
    assert expected("span_limit")[4] == (1, 0) and expected("span_limit_scaled")[4] == (0, 1)                # 64 is kept, the next double dropped
    assert expected("bad_values")[4] == (5, 1)
    assert expected("touch_no_centre")[2:6] == ((3, 1), (0, 1), (0, 0), (0, 0))                              # inside, yet no centre
    assert expected("owner_three")[1][0][1].tolist() == [-1, 2, 2, 1, 1, 1, -1]                             # the lowest id wins


def test_rectangle_rule_equals_every_cell_rule_on_random_grids():
    """the rectangle the kernel tests loses no covered centre, and no OUTSIDE disc covers one: 320 random small grids with
    integer and non-integer origins, 60 discs each, among them discs tangent to a centre (snapped to centre +- R), R = 0 on a
    centre and R = cell / 2"""
    rng = np.random.default_rng(35)
    for trial in range(320):
        nx, ny = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        cell = float(rng.choice([1.0, 0.5, 2.0, 3.0, 0.1, 0.7, 1.0 / 3.0, 12.0]))
        x0, y0 = (float(rng.integers(-50, 50)), float(rng.integers(-50, 50))) if trial % 2 == 0 else (float(rng.uniform(-50, 50)), float(rng.uniform(-50, 50)))
        grid = (x0, y0, cell, nx, ny)
        assert not cm.refused(grid)
        n = 60
        R = rng.choice([0.0, 0.5 * cell, cell, 2.5 * cell, 5.0 * cell], size=n) * rng.choice([1.0, 1.0, rng.uniform(0.1, 2.0)], size=n)
        ix, iy = rng.integers(-3, nx + 3, size=n), rng.integers(-3, ny + 3, size=n)
        cx, cy = x0 + (ix.astype(np.float64) + 0.5) * cell, y0 + (iy.astype(np.float64) + 0.5) * cell
        kind = rng.integers(0, 6, size=n)  # 0: anywhere, 1 .. 4: tangent to the centre from a side, 5: on the centre
        x = np.where(kind == 0, x0 + rng.uniform(-3, nx + 3, size=n) * cell, np.where(kind == 1, cx - R, np.where(kind == 2, cx + R, cx)))
        y = np.where(kind == 0, y0 + rng.uniform(-3, ny + 3, size=n) * cell, np.where(kind == 3, cy - R, np.where(kind == 4, cy + R, cy)))
        ids = rng.integers(1, 5, size=n)
        half = n // 2
        args = ([x[:half], x[half:]], [y[:half], y[half:]], [R[:half], R[half:]], [ids[:half], ids[half:]])
        rect, full = cm.cover(grid, 1.0, *args), cm.cover(grid, 1.0, *args, full=True)
        assert cm.same(rect, full), (trial, grid)
        # an outside disc covers no centre of the grid
        gx, gy = x0 + (np.arange(nx) + 0.5) * cell, y0 + (np.arange(ny) + 0.5) * cell
        f = cm.fate(grid, 1.0, x, y, R)[0]
        for k in np.nonzero(f == 1)[0]:
            dx, dy = gx - x[k], gy - y[k]
            assert not ((dx * dx)[None, :] + (dy * dy)[:, None] <= R[k] * R[k]).any(), (trial, grid, k)


def test_the_resolution_refusal_boundary():
    two20 = 2.0 ** 20
    assert not cm.refused((0.0, 0.0, 1.0, 1024, 1024)) and not cm.refused((-two20, 0.0, 1.0, 4, 4))
    assert not cm.refused((two20 - 4.0, 0.0, 1.0, 4, 4)) and cm.refused((two20 - 3.0, 0.0, 1.0, 4, 4))   # x0 + nx * cell one cell too far
    assert cm.refused((float(np.nextafter(-two20, -np.inf)), 0.0, 1.0, 4, 4)) and cm.refused((0.0, -two20 - 1.0, 1.0, 4, 4))
    assert not cm.refused((0.0, 0.5 * two20 - 4.0, 0.5, 8, 8)) and cm.refused((0.0, 0.5 * two20 - 3.5, 0.5, 8, 8))   # the bound scales with the cell
    assert cm.refused((1.0e9, 0.0, 1.0, 8, 8)) and not cm.refused((1.0e9, 0.0, 1024.0, 8, 8))
