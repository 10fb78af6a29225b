"""CPU tests of tests/joints_ref.py, the float64 reference of the joint coordinates and speeds that the GPU tests of the batched
joint reads compare against: hand-made poses whose answers are known."""
import math

import pytest

import joints_ref as jr


def body(px=0.0, py=0.0, angle=0.0, vx=0.0, vy=0.0, w=0.0, lc=(0.0, 0.0)):
    """a body-state row as a dict: the world centre follows from the origin, the angle and the local centre"""
    s, c = math.sin(angle), math.cos(angle)
    return {"px": px, "py": py, "angle": angle, "vx": vx, "vy": vy, "w": w,
            "cx": px + c * lc[0] - s * lc[1], "cy": py + s * lc[0] + c * lc[1]}


def test_a_slider_displaced_along_a_rotated_axis():
    # bodyA is turned by 30 degrees and its local axis is x: the world axis is (cos 30, sin 30); bodyB sits 0.75 m along it
    a = math.radians(30.0)
    A = body(2.0, 1.0, a)
    B = body(2.0 + 0.75 * math.cos(a), 1.0 + 0.75 * math.sin(a), a, vx=0.5 * math.cos(a), vy=0.5 * math.sin(a))
    jd = {"anchor_a": (0.0, 0.0), "anchor_b": (0.0, 0.0), "axis": (1.0, 0.0)}
    t, S = jr.translation(A, B, jd)
    assert t == pytest.approx(0.75, abs=1e-14)
    # the leaf terms: |pB| + |pA| per component, times the components of the axis
    assert S == pytest.approx((B["px"] + 2.0) * math.cos(a) + (B["py"] + 1.0) * math.sin(a), rel=1e-12)
    assert S >= abs(t)
    v, Sv = jr.linear_speed(A, B, jd)
    assert v == pytest.approx(0.5, abs=1e-14)
    assert Sv >= abs(v)
    # sideways motion of B does not show; anchors off the origins do
    B2 = dict(B, vx=B["vx"] - 3.0 * math.sin(a), vy=B["vy"] + 3.0 * math.cos(a))
    assert jr.linear_speed(A, B2, jd)[0] == pytest.approx(0.5, abs=1e-14)
    jd2 = {"anchor_a": (0.25, 0.0), "anchor_b": (0.0, 0.0), "axis": (1.0, 0.0)}
    assert jr.translation(A, B, jd2)[0] == pytest.approx(0.5, abs=1e-14)
    # a turning frame: B at rest 0.75 m out on an axis that turns with A at 2 rad/s neither gains nor loses translation
    A3 = dict(A, w=2.0)
    B3 = dict(B, vx=0.0, vy=0.0)
    assert jr.linear_speed(A3, B3, jd)[0] == pytest.approx(0.0, abs=1e-14)
    # ... and B moving with the frame (v = w x d) does not either
    d = (B["px"] - A["px"], B["py"] - A["py"])
    B4 = dict(B, vx=-2.0 * d[1], vy=2.0 * d[0], w=2.0)
    assert jr.linear_speed(A3, B4, jd)[0] == pytest.approx(0.0, abs=1e-14)


def test_an_off_centre_body_spinning_about_a_pin():
    # B's centre of mass lies 0.375 m from its origin; it spins at 4 rad/s about a pin at its ORIGIN, which A (at rest, axis y)
    # holds: the centre's velocity is w x (R lc), the anchor does not move, so the joint speed is 0 - but only when the local
    # centre enters: without it the reference would see the anchor move with the centre's velocity
    angle = 0.6
    lc = (0.375, 0.0)
    B = body(1.0, 2.0, angle, w=4.0, lc=lc)
    r = (B["cx"] - 1.0, B["cy"] - 2.0)
    B["vx"], B["vy"] = -4.0 * r[1], 4.0 * r[0]
    A = body(1.0, 2.0)
    jd = {"anchor_a": (0.0, 0.0), "anchor_b": (0.0, 0.0), "axis": (0.0, 1.0), "lc_b": lc}
    v, S = jr.linear_speed(A, B, jd)
    assert v == pytest.approx(0.0, abs=1e-14)
    assert S >= 4.0 * 0.375 * abs(math.cos(angle)) - 1e-12
    without = jr.linear_speed(A, B, dict(jd, lc_b=(0.0, 0.0)))[0]
    assert without == pytest.approx(B["vy"], abs=1e-14) and abs(without) > 1.0
    assert jr.translation(A, B, jd)[0] == pytest.approx(0.0, abs=1e-14)
    # an anchor out on B, 0.5 m along its x: it moves at w x (R (0.5, 0)), of which the axis y sees the y component
    jd2 = dict(jd, anchor_b=(0.5, 0.0))
    assert jr.linear_speed(A, B, jd2)[0] == pytest.approx(4.0 * 0.5 * math.cos(angle), abs=1e-14)
    assert jr.translation(A, B, jd2)[0] == pytest.approx(0.5 * math.sin(angle), abs=1e-14)


def test_a_pulley_with_both_lengths_known():
    # 3-4-5 and 5-12-13 triangles; B is turned by 90 degrees, so its local anchor (0, 1) lies at (-1, 0) from its origin
    A = body(3.0, 0.0)
    B = body(6.0, -12.0, math.pi / 2.0)
    jd = {"anchor_a": (0.0, 0.0), "anchor_b": (0.0, 1.0), "ground_a": (0.0, 4.0), "ground_b": (10.0, 0.0)}
    (la, Sa), (lb, Sb) = jr.pulley_lengths(A, B, jd)
    assert la == pytest.approx(5.0, abs=1e-14)
    assert lb == pytest.approx(13.0, abs=1e-12)
    assert Sa == pytest.approx(3.0 + 0.0 + 0.0 + 4.0 + 5.0, abs=1e-12)
    assert Sb >= 13.0
    assert jr.bound(Sa) == 32.0 * 2.0 ** -24 * Sa
