// CPU compile of the device math headers (box2d-mt_amd/csrc/b2d_*.h) for bit-level checks against
// oracle/_ref WITHOUT a GPU.  TEST INFRASTRUCTURE: nothing in the product links this file.
// (probe_cases.h holds one vector of each family; device_probe.hip runs the same cases one vector per GPU thread)
#include "probe_cases.h"
#include <math.h>

extern "C"
{

void probe_sincos(int n, const float* a, float* s, float* c)
{
	for (int i = 0; i < n; ++i)
	{
		s[i] = b2dSin(a[i]);
		c[i] = b2dCos(a[i]);
	}
}

// all five entry points per angle (caseSinCos): out8[n][8]
void probe_sincos_all(int n, const float* a, float* out8)
{
	for (int i = 0; i < n; ++i) caseSinCos(a[i], out8 + 8 * (size_t)i);
}

// exhaustive-ish check against this machine's libm over [lo, hi] bit patterns; returns mismatches
long probe_sincos_vs_libm(unsigned lo, unsigned hi, unsigned stride)
{
	long bad = 0;
	for (unsigned long u = lo; u <= hi; u += stride)
	{
		float f = b2dAsFloat((unsigned)u);
		if (f != f || f - f != 0.0f) continue;
		if (b2dAsUint(sinf(f)) != b2dAsUint(b2dSin(f))) ++bad;
		if (b2dAsUint(cosf(f)) != b2dAsUint(b2dCos(f))) ++bad;
		// the fused pair (one argument reduction for both) is what b2Rot::Set uses on the device
		float s2, c2;
		b2dSinCos(f, &s2, &c2);
		if (b2dAsUint(s2) != b2dAsUint(sinf(f)) || b2dAsUint(c2) != b2dAsUint(cosf(f))) ++bad;
	}
	return bad;
}

// shape = ShapeRec as 38 floats/ints: type, count, radius, pad, centroid(2), verts(16), normals(16)
// xf = px, py, angle ; out = 16 floats in the harness manifold layout
void probe_collide(const void* shapeA, const float* xfA, const void* shapeB, const float* xfB, float* out)
{
	caseCollide((const ShapeRec*)shapeA, xfA, (const ShapeRec*)shapeB, xfB, out);
}

void probe_shape_aabb(const void* shape, const float* xf, float* out4)
{
	caseShapeAABB((const ShapeRec*)shape, xf, out4);
}

// Same layouts as the harness probes b2h_probe_distance / b2h_probe_toi / b2h_probe_shape_cast (box2d-mt_amd/harness/harness.cpp).
void probe_distance(int countA, const float* vertsA, float radiusA, const float* xfA, int countB, const float* vertsB,
	float radiusB, const float* xfB, int useRadii, float* out6)
{
	caseDistance(countA, vertsA, radiusA, xfA, countB, vertsB, radiusB, xfB, useRadii, out6);
}

void probe_shape_cast(int countA, const float* vertsA, float radiusA, const float* xfA, int countB, const float* vertsB,
	float radiusB, const float* xfB, float tx, float ty, float* out7)
{
	const float travel[2] = { tx, ty };
	caseShapeCast(countA, vertsA, radiusA, xfA, countB, vertsB, radiusB, xfB, travel, out7);
}

// ray5 = p1, p2, maxFraction ; out4 = hit, fraction, normal
void probe_shape_raycast(const void* shape, const float* xf, const float* ray5, float* out4)
{
	caseRayCast((const ShapeRec*)shape, xf, ray5, out4);
}

int probe_test_point(const void* shape, const float* xf, const float* p2)
{
	return caseTestPoint((const ShapeRec*)shape, xf, p2);
}

// out4 = mass, center, inertia about the shape's origin
void probe_shape_mass(const void* shape, float density, float* out4)
{
	caseShapeMass((const ShapeRec*)shape, density, out4);
}

// b2dPolygonFromPoints + b2dPolygonFinish + b2dShapeMass in b2h_probe_polygon's layout: inp17 = count, 8 points
void probe_polygon(const float* inp17, float density, float* out39)
{
	casePolygon(inp17, density, out39);
}

// ownIdBlock (b2d_math.h) against the integer remainder: every block count up to `nbMax`, every `stride`-th body id below
// `bodies` plus the ids whose hash lies at the very top of its 24 bits; returns the number of mismatches
long probe_own_id_block_check(int nbMax, unsigned bodies, unsigned stride)
{
	long bad = 0;
	for (int nb = 1; nb <= nbMax; ++nb)
	{
		for (unsigned body = 0; body < bodies; body += stride)
		{
			const unsigned x = body * 2654435761u >> 8;
			if (ownIdBlock((int)body, nb) != 1 + (int)(x % (unsigned)nb)) ++bad;
		}
	}
	// (x * rcp(nb) rounds up past an integer only near the top of the 24 bits: all ids whose hash is there)
	for (unsigned body = 0; body < bodies; ++body)
	{
		const unsigned x = body * 2654435761u >> 8;
		if (x < 0xf00000u) continue;
		for (int nb = 1; nb <= nbMax; ++nb) if (ownIdBlock((int)body, nb) != 1 + (int)(x % (unsigned)nb)) ++bad;
	}
	return bad;
}

void probe_toi(int countA, const float* vertsA, float radiusA, const float* sweepA9, int countB, const float* vertsB,
	float radiusB, const float* sweepB9, float tMax, float* out2)
{
	caseToi(countA, vertsA, radiusA, sweepA9, countB, vertsB, radiusB, sweepB9, tMax, out2);
}

} // extern "C"
