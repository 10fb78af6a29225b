"""A float64 restatement of the joint getters behind b2hip_get_joint_states (include/b2hip.h, block G): the joint translation
and linear speed of a prismatic or wheel joint and the two lengths of a pulley, from body-state rows and the joint's
definition. The angular values (an angle or angular-velocity difference) are single float32 subtractions and need no reference.

Every value comes with S: the sum of the absolute values of every leaf product of the expression, expanded down to the
numbers the float32 evaluation starts from (positions, centres, sines and cosines, anchors, velocities). A float32 evaluation
of the same expression makes fewer than twenty roundings, each of a partial sum no larger than S, and starts from a stored sine
and cosine that are a few ulp from the exact ones; so it lies within 32 * 2^-24 * S of the value here.

A body is a mapping with px, py (origin), angle, cx, cy (world centre), vx, vy, w - a row of b2hip.BODY_STATE_DTYPE will do - and
a joint definition a mapping with anchor_a, anchor_b, axis (prismatic, wheel), ground_a, ground_b (pulley) and, where a body's
centre of mass is not its origin, lc_a / lc_b (the local centre; default (0, 0))."""
import math

BOUND_FACTOR = 32.0 * 2.0 ** -24


def bound(S):
    return BOUND_FACTOR * S


def _f(x):
    return float(x)


def _rot(body, v):
    """(R v, |R| |v|): the rotated vector and the sum of the absolute values of its two products per component"""
    s, c = math.sin(_f(body["angle"])), math.cos(_f(body["angle"]))
    x, y = _f(v[0]), _f(v[1])
    return (c * x - s * y, s * x + c * y), (abs(c * x) + abs(s * y), abs(s * x) + abs(c * y))


def _world_point(body, local):
    """b2Body::GetWorldPoint: (point, per-component sum of absolute leaf terms)"""
    r, ra = _rot(body, local)
    px, py = _f(body["px"]), _f(body["py"])
    return (r[0] + px, r[1] + py), (ra[0] + abs(px), ra[1] + abs(py))


def translation(body_a, body_b, jd):
    """b2PrismaticJoint::GetJointTranslation / b2WheelJoint::GetJointTranslation: dot(pB - pA, axis in the world). (value, S)"""
    pa, pa_abs = _world_point(body_a, jd["anchor_a"])
    pb, pb_abs = _world_point(body_b, jd["anchor_b"])
    axis, axis_abs = _rot(body_a, jd["axis"])
    value = (pb[0] - pa[0]) * axis[0] + (pb[1] - pa[1]) * axis[1]
    S = (pb_abs[0] + pa_abs[0]) * axis_abs[0] + (pb_abs[1] + pa_abs[1]) * axis_abs[1]
    return value, S


def linear_speed(body_a, body_b, jd):
    """b2PrismaticJoint::GetJointSpeed / b2WheelJoint::GetJointLinearSpeed:
    dot(d, cross(wA, axis)) + dot(axis, vB + cross(wB, rB) - vA - cross(wA, rA)) with r = R (anchor - local centre) and
    d = (cB + rB) - (cA + rA). (value, S)"""
    lca, lcb = jd.get("lc_a", (0.0, 0.0)), jd.get("lc_b", (0.0, 0.0))
    la = (_f(jd["anchor_a"][0]) - _f(lca[0]), _f(jd["anchor_a"][1]) - _f(lca[1]))
    lb = (_f(jd["anchor_b"][0]) - _f(lcb[0]), _f(jd["anchor_b"][1]) - _f(lcb[1]))
    la_abs = (abs(_f(jd["anchor_a"][0])) + abs(_f(lca[0])), abs(_f(jd["anchor_a"][1])) + abs(_f(lca[1])))
    lb_abs = (abs(_f(jd["anchor_b"][0])) + abs(_f(lcb[0])), abs(_f(jd["anchor_b"][1])) + abs(_f(lcb[1])))
    ra, _ = _rot(body_a, la)
    rb, _ = _rot(body_b, lb)
    _, ra_abs = _rot(body_a, la_abs)
    _, rb_abs = _rot(body_b, lb_abs)
    axis, axis_abs = _rot(body_a, jd["axis"])
    ca, cb = (_f(body_a["cx"]), _f(body_a["cy"])), (_f(body_b["cx"]), _f(body_b["cy"]))
    d = ((cb[0] + rb[0]) - (ca[0] + ra[0]), (cb[1] + rb[1]) - (ca[1] + ra[1]))
    d_abs = (abs(cb[0]) + rb_abs[0] + abs(ca[0]) + ra_abs[0], abs(cb[1]) + rb_abs[1] + abs(ca[1]) + ra_abs[1])
    wa, wb = _f(body_a["w"]), _f(body_b["w"])
    va, vb = (_f(body_a["vx"]), _f(body_a["vy"])), (_f(body_b["vx"]), _f(body_b["vy"]))
    # cross(w, v) = (-w v.y, w v.x)
    first = d[0] * (-wa * axis[1]) + d[1] * (wa * axis[0])
    first_abs = d_abs[0] * abs(wa) * axis_abs[1] + d_abs[1] * abs(wa) * axis_abs[0]
    rel = (vb[0] + (-wb * rb[1]) - va[0] - (-wa * ra[1]), vb[1] + (wb * rb[0]) - va[1] - (wa * ra[0]))
    rel_abs = (abs(vb[0]) + abs(wb) * rb_abs[1] + abs(va[0]) + abs(wa) * ra_abs[1],
               abs(vb[1]) + abs(wb) * rb_abs[0] + abs(va[1]) + abs(wa) * ra_abs[0])
    value = first + axis[0] * rel[0] + axis[1] * rel[1]
    S = first_abs + axis_abs[0] * rel_abs[0] + axis_abs[1] * rel_abs[1]
    return value, S


def _length(body, local, ground):
    p, p_abs = _world_point(body, local)
    gx, gy = _f(ground[0]), _f(ground[1])
    dx, dy = p[0] - gx, p[1] - gy
    value = math.hypot(dx, dy)
    if value == 0.0:
        return 0.0, p_abs[0] + abs(gx) + p_abs[1] + abs(gy)
    # the error of sqrt(dx^2 + dy^2) for errors ex, ey of dx, dy is (|dx| ex + |dy| ey) / length <= ex + ey; the squares, their
    # sum and the root add three roundings of the length itself
    return value, p_abs[0] + abs(gx) + p_abs[1] + abs(gy) + value


def pulley_lengths(body_a, body_b, jd):
    """b2PulleyJoint::GetCurrentLengthA / B: |GetWorldPoint(anchor) - ground anchor|. ((lengthA, S), (lengthB, S))"""
    return _length(body_a, jd["anchor_a"], jd["ground_a"]), _length(body_b, jd["anchor_b"], jd["ground_b"])
