// b2hip_api_fixtures.h - part of the ONE translation unit b2hip.hip, inside its extern "C" block: the fixtures of the C ABI of
// include/b2hip.h - create / destroy, the b2hip_fixture_* setters, and the fat AABB a new proxy gets (fatAround).
// (No include guard on purpose: b2hip.hip includes it exactly once, in order - the fragments share one scope.)

// The device record of a b2hip_shape (b2hip_create_fixture, and the query shapes of b2hip_query_shapes /
// b2hip_shape_cast_closest): nullptr, or why the shape is refused.
static const char* shapeRecordOf(const b2hip_shape* shape, ShapeRec* rec)
{
	if (shape->type != B2HIP_SHAPE_CIRCLE && shape->type != B2HIP_SHAPE_EDGE && shape->type != B2HIP_SHAPE_POLYGON && shape->type != B2HIP_SHAPE_CHAIN)
	{
		return "unknown shape type";
	}
	memset(rec, 0, sizeof(*rec));
	rec->type = shape->type;
	rec->count = shape->count;
	rec->radius = shape->radius;
	rec->centroid = v2(shape->centroid[0], shape->centroid[1]);
	int nv = shape->type == B2HIP_SHAPE_POLYGON ? shape->count : (B2D_IS_SEGMENT(shape->type) ? 4 : 1);
	if (nv > B2D_MAX_POLY_VERTS) return "too many polygon vertices";
	for (int i = 0; i < nv; ++i)
	{
		rec->verts[i] = v2(shape->verts[2 * i], shape->verts[2 * i + 1]);
		if (shape->type == B2HIP_SHAPE_POLYGON) rec->normals[i] = v2(shape->normals[2 * i], shape->normals[2 * i + 1]);
	}
	return nullptr;
}

// The fat AABB of a proxy made or moved at a shape's AABB (b2DynamicTree::CreateProxy / MoveProxy, b2DynamicTree.cpp:105-119)
static void fatAround(const AABB& aabb, float out4[4])
{
	out4[0] = aabb.lo.x - B2D_AABB_EXTENSION;
	out4[1] = aabb.lo.y - B2D_AABB_EXTENSION;
	out4[2] = aabb.hi.x + B2D_AABB_EXTENSION;
	out4[3] = aabb.hi.y + B2D_AABB_EXTENSION;
}

int b2hip_create_fixture(b2hip_world* w, int body, const b2hip_fixture_def* def, const b2hip_shape* shape)
{
	if (!w || !def || !shape) return setError(B2HIP_ERR_INVALID, "null argument");
	if (int rcu = checkUsable(w, "b2hip_create_fixture", true)) return rcu;
	if (body < 0 || body >= (int)w->bodies.size()) return setError(B2HIP_ERR_INVALID, "bad body id");
	ShapeRec rec;
	if (const char* why = shapeRecordOf(shape, &rec)) return setError(B2HIP_ERR_INVALID, why);
	HostBody& b = editBody(w, body);
	HostFixture f;
	memset(&f, 0, sizeof(f));
	f.body = body;
	f.shape = internShape(w, rec);
	f.density = def->density;
	f.friction = def->friction;
	f.restitution = def->restitution;
	f.categoryBits = def->category_bits;
	f.maskBits = def->mask_bits;
	f.groupIndex = def->group_index;
	f.isSensor = def->is_sensor != 0;
	f.thick = def->thick_shape != 0;
	// b2Fixture::CreateProxies (b2Fixture.cpp:126-141) + b2DynamicTree::CreateProxy (b2DynamicTree.cpp:105-119)
	fatAround(b2dShapeAABB(&rec, hostXf(b)), f.fat);
	const bool bodyActive = (b.flags & BF_ACTIVE) != 0;
	if (bodyActive)
	{
		f.proxyKey = allocProxyKey(w);
		if (f.proxyKey < 0) return setError(B2HIP_ERR_UNSUPPORTED, "proxy id reuse after the broad-phase tree was emptied is not modelled");
	}
	else
	{
		// (b2Body.cpp:199-203: an inactive body's fixtures get their proxies when it is activated)
		f.proxyKey = -1;
		f.noProxy = true;
	}
	const int id = (int)w->fixtures.size();
	w->fixtures.push_back(f);
	b.fixtures.push_back(id);
	if (bodyActive) w->pendingMoves.push_back(id);
	if (f.density > 0.0f) resetMassData(w, b);
	w->newFixture = true;
	return id;
}

// b2Fixture::DestroyProxies (b2Fixture.cpp:143-157) + the host bookkeeping of a fixture that is gone
static void dropFixture(b2hip_world* w, int fixture)
{
	HostFixture& f = w->fixtures[fixture];
	freeProxyKey(w, f.proxyKey);
	f.dead = true;
	w->proxyEdits.push_back(fixture);
	w->proxyListsStale = true;
	// (a proxy created since the last step and not yet buffered on the device leaves the pending moves too: UnBufferMove)
	w->pendingMoves.erase(std::remove(w->pendingMoves.begin(), w->pendingMoves.end(), fixture), w->pendingMoves.end());
}

int b2hip_destroy_fixture(b2hip_world* w, int fixture)
{
	if (int rc = checkFixture(w, fixture, "b2hip_destroy_fixture")) return rc;
	const int body = w->fixtures[fixture].body;
	HostBody& b = editBody(w, body);
	queueOp(w, EDIT_DESTROY_FIXTURE, fixture);
	b.fixtures.erase(std::remove(b.fixtures.begin(), b.fixtures.end(), fixture), b.fixtures.end());
	dropFixture(w, fixture);
	resetMassData(w, b);
	return B2HIP_OK;
}

int b2hip_fixture_is_destroyed(const b2hip_world* w, int fixture)
{
	return w && fixture >= 0 && fixture < (int)w->fixtures.size() && w->fixtures[fixture].dead ? 1 : 0;
}

int b2hip_fixture_set_sensor(b2hip_world* w, int fixture, int is_sensor)
{
	if (int rc = checkFixture(w, fixture, "b2hip_fixture_set_sensor")) return rc;
	HostFixture& f = w->fixtures[fixture];
	if (f.isSensor == (is_sensor != 0)) return B2HIP_OK;
	setAwake(w, f.body);
	f.isSensor = is_sensor != 0;
	w->proxyEdits.push_back(fixture);
	queueOp(w, EDIT_SENSOR_FIXTURE, fixture);
	queueOp(w, EDIT_RECALC_FIXTURE, fixture);
	return B2HIP_OK;
}

int b2hip_fixture_set_thick(b2hip_world* w, int fixture, int thick_shape)
{
	if (int rc = checkFixture(w, fixture, "b2hip_fixture_set_thick")) return rc;
	HostFixture& f = w->fixtures[fixture];
	if (f.thick == (thick_shape != 0)) return B2HIP_OK;
	f.thick = thick_shape != 0;
	w->proxyEdits.push_back(fixture);
	queueOp(w, EDIT_RECALC_FIXTURE, fixture);
	return B2HIP_OK;
}

int b2hip_fixture_refilter(b2hip_world* w, int fixture)
{
	if (int rc = checkFixture(w, fixture, "b2hip_fixture_refilter")) return rc;
	queueOp(w, EDIT_REFILTER_FIXTURE, fixture);
	w->refilterPending = true;
	// TouchProxy (b2BroadPhase.cpp:70-73): the proxy is buffered as moved so that new pairs can form
	if (w->bodies[w->fixtures[fixture].body].flags & BF_ACTIVE) w->pendingMoves.push_back(fixture);
	return B2HIP_OK;
}

int b2hip_fixture_set_filter(b2hip_world* w, int fixture, uint16_t category_bits, uint16_t mask_bits, int16_t group_index)
{
	if (int rc = checkFixture(w, fixture, "b2hip_fixture_set_filter")) return rc;
	HostFixture& f = w->fixtures[fixture];
	f.categoryBits = category_bits;
	f.maskBits = mask_bits;
	f.groupIndex = group_index;
	w->proxyEdits.push_back(fixture);
	return b2hip_fixture_refilter(w, fixture);
}

// b2Fixture::SetDensity / SetFriction / SetRestitution (b2Fixture.h:306-334): plain values - the density is read by the next
// ResetMassData, friction and restitution by the contacts created from now on (existing contacts keep their mixture)
int b2hip_fixture_set_material(b2hip_world* w, int fixture, float density, float friction, float restitution)
{
	if (int rc = checkFixture(w, fixture, "b2hip_fixture_set_material")) return rc;
	HostFixture& f = w->fixtures[fixture];
	f.density = density;
	f.friction = friction;
	f.restitution = restitution;
	w->proxyEdits.push_back(fixture);
	return B2HIP_OK;
}

