"""The ground-truth world: a camera that looks at a triangle mesh, not at the NeRF (DESIGN.md "The ground-truth world").

The reference's second simulator (validation/simulators/BlenderSimulator.py:82,102) hands the estimator an image of the TRUE world
(Agent.get_img, a Blender subprocess); the NeRF is only the drone's model of it.  MeshWorld is that camera without Blender: rays from
nerf.utils.get_rays (so a world frame and a NeRF frame of one pose are pixel-aligned) cast against a mesh, shaded by a headlight.

    MeshWorld(vertices, faces, colors=None, resolution=None, frame="nerf")
        .cast(rays_o, rays_d, t_min=0.0, t_max=inf, frame_width=None)  -> {"t", "prim", "u", "v"}
        .shade(rays_d, hit, bg_color=1.0, ambient=0.3)                 -> (image float32 [...,3], image_u8 uint8 [...,3])
        .render(pose, intrinsics, H, W, bg_color=1.0)                  -> {"image", "image_u8", "depth", "prim"}

A mesh on a HIP device goes through csrc/raycast.hip (a uniform grid, one lane per ray) on the current stream; a CPU tensor or a numpy
array through numpy: brute force over all triangles, chunked -- the package's CPU implementation, as mesh.isosurface has one.

This docstring is the specification of every rule below; csrc/raycast.hip, csrc/overlay.hip, csrc/voxelize.hip, csrc/closest.hip, csrc/body.hip,
csrc/clearance.hip and DESIGN.md point here, and a change to a rule is made in this text, in the numpy path and in the kernel.

The hit rule; both paths implement it in float32 with one rounding per operation, so they agree bit for bit:
    per triangle v0, e1 = v1 - v0, e2 = v2 - v0;  p = d x e2, det = e1 . p, reject det == 0, inv = 1 / det, s = o - v0,
    u = (s . p) * inv, q = s x e1, v = (d . q) * inv, t = (e2 . q) * inv;  a . b = (ax bx + ay by) + az bz,
    (a x b).x = ay bz - az by (and cyclic);  accept iff u >= 0 and v >= 0 and u + v <= 1 and t_min < t < t_max (NaN fails);
    the closest hit is the smallest t, equal t goes to the lowest triangle index; a ray with a non-finite component or a zero
    direction misses.  A miss is t = +inf, prim = -1, u = v = 0.
The grid only chooses which triangles a ray is tested against: no result depends on it, nor on frame_width.

Shading, float32, one rounding per operation: colour = (((1 - u) - v) c0 + u c1) + v c2 of the hit triangle's vertex colours (mid-grey
    without), times the headlight ambient + (1 - ambient) c, c = min(|n . d| / len, 1) with len = sqrt(n . n) sqrt(d . d) and c = 0
    unless len > 0 -- two-sided, n = e1 x e2 and d as they are, not normalised -- clamped to [0, 1]; a miss is the background.  The
    uint8 copy of a pixel is (uint8)(clamp(x, 0, 1) * 255).  The overlay's pixels take the same headlight, on the hit's normal, and
    the same uint8 copy.

The grid rule (grid_params): the vertices' bounding box padded by ext / 128 + S / 1024 on every side (ext its largest extent, S the
largest of ext and the largest coordinate magnitude); `resolution=None` picks n_a = round(size_a * cbrt(4 F / volume)) cells on axis
a, clamped to 1..256 -- about four cells per triangle, cells near cubic; a triangle's bounding box is grown by
max(cell / 32, S / 4096) on every side before it is binned, and rays whose origin lies beyond 64 S walk no grid (all triangles).

The world is also the truth a rollout's collisions are judged against (DESIGN.md "The ground-truth collision field"): the reference's
collision map comes from the scene's mesh (validation/utils/createCollisionMap.py), not from the NeRF.  That script marks the cells that
hold a mesh vertex, which leaves holes wherever a triangle is larger than a cell; here every cell a triangle touches is marked.

        .occupancy(box, rot=PLANNER_ROT)                               -> bool [X,Y,Z] on the world's device
    voxelize_numpy(vertices_world, faces, box, all_cells=False)        -> bool [X,Y,Z] numpy

A mesh on a HIP device goes through csrc/voxelize.hip on the current stream, a CPU world through voxelize_numpy; the two maps are equal.

The voxelisation rule (written here once, implemented in voxelize_numpy and in csrc/voxelize.hip):
    inputs: the world's vertices (float32, the NeRF's axes; the exact vertices, not tri_data: v0 + e1 is not v1) and faces, a
    collision.GridBox, and rot -- a signed permutation matrix (entries 0 or +-1, one per row and column; anything else is a ValueError),
    so that the inverse of collision.to_nerf, w_i = sum_j rot[i][j] x_j, is a copy or a negation: no rounding.
    Everything after the permutation is float64, one IEEE rounding per operation, no contraction;  a . b = (ax bx + ay by) + az bz,
    (a x b).x = ay bz - az by (and cyclic).
    Cell (i, j, k) has the centre c_a = start_a + (i_a + 0.5) / g and the half-width h = 0.5 / g, g the box's granularity.
    A cell is occupied iff at least one face (v0, v1, v2) satisfies (a) or (b):
    (a) the closed triangle-box separating-axis test (Akenine-Moeller's 13 axes) finds no separating axis.  With the edges
        e0 = v1 - v0, e1 = v2 - v1, e2 = v0 - v2 and the normal n = e0 x e1 (of the world vertices: the same for every cell) and the
        shifted vertices v_k' = v_k - c:
            box axis a       separates iff  min_k v'_ka > h  or  max_k v'_ka < -h
            the normal       separates iff  |n . v_0'| > h ((|nx| + |ny|) + |nz|)
            a = u_i x e_j    separates iff  min_k p_k > r  or  max_k p_k < -r,  p_k = a . v_k',  r = h ((|ax| + |ay|) + |az|)
        (u_0 x e = (0, -ez, ey), u_1 x e = (ez, 0, -ex), u_2 x e = (-ey, ex, 0): the zero component drops out of both sums exactly).
        All inequalities are strict, so touching is overlap; a zero axis separates nothing, so a zero-area face is decided by the
        remaining axes -- conservative.
    (b) one of the face's three vertices lies in the cell by GridBox.indices' rule, floor((w_a - start_a) g) in float64, inside the box
        -- so the map is a superset of collision.occupancy_from_points on the vertices the faces use.
    Candidates: the result is defined over all cells of the box; an implementation may test any superset of the overlapping cells.
    Both test, per axis, the cells floor((min_k w_ka - start_a) g) - 1 .. floor((max_k w_ka - start_a) g) + 1, clipped to the box
    (face_candidates); voxelize_numpy(all_cells=True) tests every cell of the box instead, and gives the same map.

The world also judges a BODY, not only a point (DESIGN.md "Body collision"): the reference's verdict, SignedDistanceField.lookup's
value < 1 / granularity, is true only when the drone's CENTRE lies in an occupied cell (the field is a distance transform in whole cells:
a neighbour's value is exactly 1 / granularity, not below it).  A rotor arm through a pillar is then no failure.  Opt-in, a stress test
judges the planner's body box instead (collision.BodyBox, body_boxes), against the mesh's triangles or against a map's occupied cells.

        .box_overlap(boxes, rot=PLANNER_ROT)                           -> {"prim": int32 [N]} on the world's device
    box_overlap_numpy(boxes, vertices_world, faces)                    -> the same, numpy: brute force over all (box, face) pairs
    collision.box_cells(boxes, occupied, box)                          -> int32 [N]; collision.box_cells_numpy is its numpy path

A HIP world / a map on a HIP device goes through csrc/body.hip (one wave per box) on the current stream, anything else through the
numpy paths; the two agree bit for bit.

The body rule (written here once; box_tri_overlap / collision.box_cell_overlap and csrc/body.hip implement it):
    The box table: boxes float64 [N,15]; a row is the centre c (3), R row-major (9) and the half extents h (3).  The COLUMNS of R
    are the box's axes in the world frame (the frame of collision.GridBox and of the rollout's states).  No kernel and no numpy
    path computes a rotation: R comes from collision.body_boxes, the one place Rodrigues' formula is evaluated for this rule.
    Everything is float64, one IEEE rounding per operation, no contraction, with the a . b and a x b of the voxelisation rule.
    A row with a non-finite entry or a negative half extent overlaps nothing.  Every inequality below is evaluated as written: "all
    p_k > r" is three comparisons, not a minimum, so a NaN (the overflow of an absurd box) fails it and separates nothing.
    Into the box's frame: x' = R^T (x - c), summed as x'_a = (R_0a d_0 + R_1a d_1) + R_2a d_2 with d = x - c.
    Box against a triangle -- exact and closed.  The world vertices are formed as the voxelisation forms them (the exact float32
        vertices through the signed permutation rot, no rounding), taken to the box's frame, v_k' (k = 0, 1, 2), and tested by the
        voxelisation's rule (a) with one half-width per axis; the edges e0 = v1' - v0', e1 = v2' - v1', e2 = v0' - v2' and the normal
        n = e0 x e1 are those of the v_k':
            box axis a       separates iff  all v'_ka > h_a  or  all v'_ka < -h_a
            the normal       separates iff  |n . v_0'| > (h_x |n_x| + h_y |n_y|) + h_z |n_z|
            a = u_i x e_j    separates iff  all p_k > r  or  all p_k < -r,  p_k = a_b v'_kb + a_c v'_kc,  r = h_b |a_b| + h_c |a_c|
        over the two components b < c that are not identically zero (u_0 x e = (0, -ez, ey), u_1 x e = (ez, 0, -ex), u_2 x e =
        (-ey, ex, 0)).  Strict inequalities: touching is overlap; a zero axis separates nothing (a zero-area face is decided by the
        remaining axes).  prim of a box = the LOWEST index of an overlapping face, or -1 -- the minimum, so that a triangle listed
        in several grid cells is harmless: no deduplication, no atomics.
        The grid only chooses candidates: an implementation may test any superset of the overlapping triangles, and no result
        depends on the grid.  csrc/body.hip takes the grid cells reached by the box's world bounds c_a -+ E_a, E_a = (|R_a0| h_0 +
        |R_a1| h_1) + |R_a2| h_2, permuted into the mesh's axes, rounded outward to float32 and grown by the binning's growth; the
        cell arithmetic floor((x - lo) * inv_cell) is non-decreasing in x and binning applies the same to a triangle's grown bounds,
        so a triangle that shares a point with the box's bounds is listed in a cell of the range (the argument in full: body.hip).
    Box against a map's cells.  occupied bool [X,Y,Z] on a GridBox; cell (i, j, k) is the cube with the centre m = start +
        ((i, j, k) + 0.5) / g and the half-width s = 0.5 / g (the voxelisation's cell).  It overlaps the box iff the closed 15-axis
        box-box separating-axis test finds no separating axis, evaluated in the box's frame, where the box is axis-aligned and the
        cell's axis i is ROW i of R; with t = m' (the centre in the box's frame) and A_ia = |R_ia|:
            box axis a            separates iff  |t_a| > h_a + s ((A_0a + A_1a) + A_2a)
            cell axis i           separates iff  |(R_i0 t_0 + R_i1 t_1) + R_i2 t_2| > ((h_0 A_i0 + h_1 A_i1) + h_2 A_i2) + s
            u_a x (row i)         separates iff  |R_ib t_c - R_ic t_b| > (h_b A_ic + h_c A_ib) + s (A_ja + A_ka)
        with (a, b, c) and (i, j, k) cyclic: b = a + 1, c = a + 2, j = i + 1, k = i + 2 (mod 3).  Strict inequalities; a zero cross
        axis separates nothing.  (The last term uses (row i x row j) = +- row k, true of a rotation; R is used as given.)
        cell of a box = the LOWEST C-order linear index (i Y + j) Z + k of an occupied overlapping cell, or -1.  Cells outside the
        array do not exist: the part of a body that sticks out of the map touches nothing, as the IndexError branch of the reference's
        lookup has it.  lookup's wrap of a negative index (numpy's indexing) is NOT reproduced here.
        Candidates: any superset; both paths take, per axis, the cells floor((c_a - E_a - start_a) g) - 1 .. floor((c_a + E_a -
        start_a) g) + 1 clipped to the map; collision.box_cells_numpy(all_cells=True) tests every cell, and gives the same result.

The verdict says whether the body touches; a stress test that adapts -- the Cross Entropy Method's risk -- wants to know HOW NEAR it came
(DESIGN.md "Body clearance"): the gap between the body box and the nearest obstacle, continuous in the pose, zero exactly when the
verdict says collision, measured on the verdict's geometry.  Opt-in (clearance= on the simulators):

        .box_clearance(boxes, max_distance=inf, rot=PLANNER_ROT)       -> {"distance" float64 [N], "prim" int32 [N], "hit" int32 [N]}
    box_clearance_numpy(boxes, vertices_world, faces, max_distance)    -> the same, numpy: brute force over all (box, face) pairs
    box_tri_distance2(boxes, tri)                                      -> the rule's squared distance per (box, face) pair
    collision.box_cells_clearance(boxes, occupied, box, max_distance)  -> {"distance", "cell", "hit"}; box_cells_clearance_numpy is its
                                                                          numpy path, collision.box_cell_distance2 the pair's d2
    collision.trajectory_clearance(states, body, world= / sdf=, ...)   -> the same for recorded drone states [n, 6]

A HIP world / a map on a HIP device goes through csrc/clearance.hip (one wave per box) on the current stream, anything else through the
numpy paths; the two agree bit for bit.

The clearance rule (written here once; box_tri_distance2 / collision.box_cell_distance2 and csrc/clearance.hip implement it):
    The body rule's box table, frame and arithmetic: float64, one IEEE rounding per operation, correctly rounded / and sqrt, no
    contraction, a . b = (a_0 b_0 + a_1 b_1) + a_2 b_2.  Everything happens in the box's frame (x' = R^T (x - c), as above), where the
    box is the axis-aligned [-h, h].  Per pair a squared distance d2: the smallest of a fixed list of candidates, starting from
    +inf, a candidate replacing the best so far only when strictly smaller -- so a NaN never replaces, and the order of the
    candidates decides nothing.  clamp01(x): x = 0 unless x >= 0, then x = 1 unless x <= 1 (a NaN becomes 0).
    A point against the box, gap2(x, h):  g_a = |x_a| - h_a where that is > 0, else 0;  d2 = (g_0^2 + g_1^2) + g_2^2.
    A box edge against a segment, edge2(a, sb, sc; q0, q1): the box edge along axis a through (sb h_b, sc h_c) (b = a + 1, c = a + 2
        mod 3; sb, sc = -1 or +1) is p1 + s L u_a, 0 <= s <= 1, with p1_a = -h_a, p1_b = sb h_b, p1_c = sc h_c, L = h_a + h_a; the
        segment is q0 + t w, w = q1 - q0.  The clamped closed form, with the box edge's dots reduced to their one non-zero term:
            r = p1 - q0;  A = L L,  e = w . w,  f = w . r,  c = L r_a,  b = L w_a,  den = A e - b b
            s0 = clamp01((b f - c e) / den) when den > 0, else 0            (parallel or degenerate: any s is as near; 0 is taken)
            t0 = (b s0 + f) / e;   low = (e == 0) or not (t0 >= 0);   high = not low and t0 > 1
            t  = 0 when low, 1 when high, else t0                           (e == 0: the segment is a point, t = 0; a NaN t0 is low)
            s  = s0 when neither, else 0 when A == 0, else clamp01((-c when low, b - c when high) / A)       (A == 0: the edge is a point)
            d_a = (p1_a + L s) - (q0_a + w_a t),  d_b = p1_b - (q0_b + w_b t),  d_c likewise;  d2 = (d_0^2 + d_1^2) + d_2^2
        The twelve box edges: a = 0, 1, 2 and (sb, sc) = (-, -), (+, -), (-, +), (+, +).
    Box against a triangle, on the body rule's v_k' (the exact float32 vertices taken to float64, in the box's frame):
        d2 = 0 if the body rule's closed 13-axis test says overlap.  Otherwise the smallest of 47 candidates:
            1. the 3 vertices against the box: gap2(v_k', h)
            2. the 8 box corners (+-h_0, +-h_1, +-h_2) against the triangle, by the closest-point rule's d2 (interior candidate, then
               the three segments; closest_terms in float64, defined for zero-area faces), with the v_k' as its vertices
            3. the 3 triangle edges v0' -> v1', v1' -> v2', v2' -> v0' against the 12 box edges: edge2
        Two disjoint convex bodies are nearest at a vertex-face or an edge-edge pair -- an edge-face or face-face contact holds
        one of those -- so the candidates are complete; penetration is the overlap test's case (no depth: an overlapping body is 0).
    Box against a map's cell (the body rule's cell: centre m, half-width s = 0.5 / g, axes the world's):
        d2 = 0 if the body rule's closed 15-axis test says overlap.  Otherwise the smallest of 160 candidates:
            1. the 8 cell corners x = m + (+-s, +-s, +-s) against the box: gap2(x', h)
            2. the 8 box corners against the cell: y_i = (c_i + ((R_i0 o_0 + R_i1 o_1) + R_i2 o_2)) - m_i with o_a = +-h_a;
               gap2(y, (s, s, s))
            3. the 12 cell edges -- along world axis i from x0 to x1, x0_i = m_i - s, x1_i = m_i + s, the other two coordinates
               m_j +- s, m_k +- s -- as segments x0' -> x1' against the 12 box edges: edge2
    Per box:
        hit  = the lowest index of a candidate that overlaps, or -1: box_overlap's prim / box_cells' cell -- the same test function.
        d2   = the smallest over the box's candidates; an equal d2 goes to the lowest index, and where hit >= 0 the index is hit.
        distance = sqrt(d2), accepted iff distance <= max_distance (+inf is allowed; NaN or a value <= 0 is a ValueError).
        A box with no accepted candidate, or an invalid row (a non-finite entry, a negative half extent): distance = +inf, prim (cell)
        = hit = -1.  Cells outside the array do not exist.
    Candidates: any superset; no result depends on them.  csrc/clearance.hip takes body.hip's ranges with E_a + max_distance in E_a's
        place: for the mesh the grid cells reached by c_a -+ (E_a + max_distance) after the same outward rounding, growth and cell
        arithmetic (a triangle within max_distance of the box has a point within max_distance of the box's bounds on every axis); for a
        map the cells floor((c_a -+ (E_a + max_distance) - start_a) g) -+ 1, clipped.
        The skip.  A pair may be left out when the gap between its bounds and the box proves that it can neither win, nor tie, nor be
        accepted: with lo_a .. hi_a the bounds of the triangle's v_k' (of the cell: t_a -+ s ((A_0a + A_1a) + A_2a)) in the box's frame,
        lb2 = gap2-style (max(lo_a - h_a, -h_a - hi_a, 0) per axis), m = sum_a (max(|lo_a|, |hi_a|) + h_a) and `bound` the smaller of
        max_distance^2 and any d2 found so far for the box, the pair is skipped iff lb2 > bound + 2^-40 (bound + m^2).  Every
        candidate is the squared distance of a point of the box and a point of the triangle (cell) computed with a few roundings of
        coordinates no larger than m, so it is at least lb2 less 2^-47 (d2 + m^2): the margin is 2^7 times the rounding.  Every
        min and max of the bounds (and of the closest-point rule's box2) is numpy's: a NaN operand is the result, in the kernels too
        (not fmin / fmax, which drop it), so a NaN coordinate reaches the comparison, fails it, and never skips.  An overlapping pair has lb2 within that rounding of 0 and is never skipped.  The numpy paths skip on
        max_distance^2 only (brute force otherwise), the kernels on both; all_cells=True tests every cell of the map.

The world can also be drawn with analytic primitives in it -- the replay's failure view (replay.failure_view; DESIGN.md "Failure
replay"), in the place of the Blender scene of validation/utils/viz_failures_blend.py:

        .cast_overlay(rays_o, rays_d, prims, t_max=None, t_min=0.0, frame_width=None)   -> {"t", "prim", "normal"}
        .render_scene(pose, intrinsics, H, W, tubes=(), boxes=(), ...)                  -> render's dict + "overlay_prim"
    overlay_prims(tubes, boxes)                                                         -> (prims float32 [P,8], colors float32 [P,3])

A HIP world goes through csrc/overlay.hip, a CPU world through cast_overlay_numpy; the two agree bit for bit.  The primitive table
holds 8 floats per primitive: kind, a.xyz, b.xyz, r -- kind 0 a capsule with the axis a-b and the radius r (a polyline of n points is
n - 1 capsules), kind 1 an axis-aligned box with the centre a and the half extents b (r is not used by the rule).  Any other kind, a
non-finite field or r <= 0 is a ValueError.  The overlay's hit rule per (ray, primitive), float32, one rounding per operation
(correctly rounded division and square root):
    x . y = (x0 y0 + x1 y1) + x2 y2;  (x X y)_0 = x1 y2 - x2 y1 (and cyclic);  dd = d . d (d is not normalised), inv_dd = 1 / dd
    re-centring on a point c: t0 = (d . (c - o)) inv_dd, o' = o + t0 d, p = o' - c;  an intersection is solved for o' and reported
        as t = t0 + t' (the cancellation of the quadratics scales with the primitive's size, not the camera's distance)
    capsule: ba = b - a, baba = ba . ba, rr = r r; three candidates t in this order, a later one replaces an earlier one only when
        strictly smaller:
        body      re-centred on m = (a + b) * 0.5: oa = p + (m - a);  u = ba X d, w = ba X oa, A = u . u, B = u . w,
                  C = w . w - rr baba, h = B B - A C;  iff A > 0 and h >= 0: t' = (-B - sqrt(h)) / A, y = ba . oa + t' (ba . d);
                  a candidate iff 0 < y < baba;  normal (oa + t' d) baba - ba y
        cap at a  re-centred on a itself:  Bs = d . p, Cs = p . p - rr, hs = Bs Bs - dd Cs;  iff hs >= 0:
                  t' = (-Bs - sqrt(hs)) / dd;  normal p + t' d
        cap at b  the same, re-centred on b (two capsules of a polyline compute the same bits for their joint: it goes to the lower)
        (nearer roots only: their smallest is where the line enters the capsule, so a ray that starts inside sees nothing of it;
        a == b gives A = 0, a sphere)
    box: re-centred on a; per axis k with d_k != 0: inv = 1 / d_k, t1 = (-b_k - p_k) inv, t2 = (b_k - p_k) inv, near = min, far = max;
        with d_k == 0 a miss iff |p_k| > b_k, else unconstrained;  t' = the largest near (the first axis that attains it gives the
        normal: its unit vector against d), a hit iff t' <= the smallest far
    acceptance: accept iff t > t_min and t < t_max[ray] (NaN fails); the smallest t wins, equal t goes to the lowest primitive index;
        a ray with a non-finite component or a zero direction is a miss: t = +inf, prim = -1, normal = 0.
    t_max[ray] is the mesh cast's t of the same ray (+inf on a mesh miss): the depth merge with the world is part of the cast.

The world is also what the NeRF's exported surface is measured against (mesh.surface_error; DESIGN.md "Surface error"): the closest
point of the mesh to every query point.

        .closest(points, max_distance=inf, coherent=None)              -> {"distance", "prim", "point"}
    closest_numpy(points, vertices, faces, max_distance=inf)           -> the same, numpy: brute force over all triangles

A HIP world goes through csrc/closest.hip (the cast's grid, one lane per point) on the current stream, a CPU world through
closest_numpy; the two agree bit for bit.

The closest-point rule; float32, one rounding per operation (correctly rounded division and square root), the hit rule's a . b and
a x b.  It is defined on the EXACT vertices v0, v1, v2 = vertices[faces] (not tri_data: v0 + e1 is not v1), e1 = v1 - v0,
e2 = v2 - v0, for every input, zero-area faces included.  Per (point p, triangle) the smallest of four candidate squared distances,
in this order, a later candidate replacing an earlier one only when strictly smaller (NaN never replaces):
    interior    n = e1 x e2, nn = n . n, s = p - v0, sn = s . n, b = ((s x e2) . n) / nn, c = ((e1 x s) . n) / nn;
                a candidate iff nn > 0 and b >= 0 and c >= 0 and b + c <= 1 (NaN fails);
                d2 = the larger of (sn sn) / nn and box2 (box2 when the first is NaN), box2 = g . g the squared distance from p to
                the triangle's bounding box, g_a = max(max(min_k v_ka - p_a, p_a - max_k v_ka), 0) -- in exact arithmetic box2 is never
                the larger; in float32 it keeps a sliver's cancellation from reporting a far triangle as near, which is what lets
                the search below stop;  closest point p - (sn / nn) n
    segments    v0 -> v1, v0 -> v2, v1 -> v2 (ab = e1, e2, v2 - v1; ap = s, s, p - v1):  den = ab . ab, x = (ap . ab) / den,
                t = 0 when den == 0, else x;  then t = 0 unless t >= 0, t = 1 unless t <= 1;  r = ap - t ab, d2 = r . r;
                closest point a + t ab, and b itself when t == 1 (so the closest point of a vertex is that vertex, bit for bit)
    Across triangles the smallest d2 below +inf wins, an equal d2 goes to the lowest triangle index.
    acceptance: distance = sqrt(d2) <= max_distance (+inf is allowed; NaN is a ValueError), max_distance rounded to float32.
    A point with a non-finite component, or without an accepted triangle, is a miss: distance = +inf, prim = -1, point = NaN.
The grid only chooses which triangles a point is tested against: no result depends on it, nor on `coherent` (the HIP path sorts
the queries by grid cell before the launch and scatters the results back: a wave's lanes then search the same cells).
A point with a component beyond REACH S is tested against every triangle.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .collision import PLANNER_ROT, to_nerf

MAX_CELLS_PER_AXIS = 256
PAD_EXTENT, PAD_SCALE = 2.0 ** -7, 2.0 ** -10       # padding of the grid box: ext * PAD_EXTENT + S * PAD_SCALE
GROW_CELL, GROW_SCALE = 2.0 ** -5, 2.0 ** -12       # growth of a triangle's box at binning: max(cell * GROW_CELL, S * GROW_SCALE)
REACH = 64.0                                        # rays starting beyond REACH * S are tested against every triangle
CELLS_PER_TRIANGLE = 4.0                            # the automatic resolution's target
DEFAULT_AMBIENT = 0.3
GREY = 0.5
_CHUNK_PAIRS = 1 << 20                              # (ray, triangle) pairs per chunk of the numpy path
_VOXEL_CHUNK_PAIRS = 1 << 18                        # (face, candidate cell) pairs per chunk of voxelize_numpy
_CLOSEST_CHUNK_PAIRS = 1 << 19                      # (point, triangle) pairs per chunk of closest_numpy
COHERENT_MIN_POINTS = 1 << 15                       # MeshWorld.closest(coherent=None) sorts the queries by cell from here on
MAX_PAIRS_PER_LAUNCH = 2 ** 31 - 1                  # ngp_voxelize_mark: pairs per call; a mesh with more is marked in several calls

_f32 = np.float32


# ------------------------------------------------------------------------------------------------------------- the grid (host)
def grid_params(vmin, vmax, n_faces, resolution=None):
    """the grid of a mesh with bounding box vmin..vmax (float32 [3]) and n_faces triangles -> dict of float32 arrays lo, cell,
    inv_cell, grow [3], float32 reach, int n [3].  All of it float32 host arithmetic, shared by the kernels and the numpy binning."""
    vmin, vmax = np.asarray(vmin, _f32), np.asarray(vmax, _f32)
    ext = _f32((vmax - vmin).max())
    S = _f32(max(ext, np.abs(vmin).max(), np.abs(vmax).max()))
    if not S > 0:
        S = _f32(1.0)
    pad = _f32(ext * _f32(PAD_EXTENT) + S * _f32(PAD_SCALE))
    lo = (vmin - pad).astype(_f32)
    size = ((vmax + pad) - lo).astype(_f32)
    if resolution is None:
        k = np.cbrt(CELLS_PER_TRIANGLE * max(1, int(n_faces)) / float(np.prod(size.astype(np.float64))))
        n = np.clip(np.rint(size.astype(np.float64) * k), 1, MAX_CELLS_PER_AXIS).astype(np.int64)
    else:
        n = np.asarray(resolution, dtype=np.int64).reshape(-1)
        if n.size == 1:
            n = np.repeat(n, 3)
        if n.shape != (3,) or (n < 1).any():
            raise ValueError(f"MeshWorld: resolution is one or three positive cell counts (got {resolution})")
        if (n > MAX_CELLS_PER_AXIS).any():
            raise ValueError(f"MeshWorld: at most {MAX_CELLS_PER_AXIS} cells per axis (got {tuple(int(v) for v in n)})")
    cell = (size / n.astype(_f32)).astype(_f32)
    inv_cell = (_f32(1.0) / cell).astype(_f32)
    grow = np.maximum(cell * _f32(GROW_CELL), S * _f32(GROW_SCALE)).astype(_f32)
    return {"lo": lo, "cell": cell, "inv_cell": inv_cell, "grow": grow, "reach": _f32(_f32(REACH) * S), "n": n}


def _grid_struct(g):
    s = _lib.RaycastGrid()
    for a in range(3):
        s.lo[a], s.cell[a], s.inv_cell[a], s.grow[a], s.n[a] = float(g["lo"][a]), float(g["cell"][a]), float(g["inv_cell"][a]), float(g["grow"][a]), int(g["n"][a])
    s.reach = float(g["reach"])
    return s


def pack_triangles(vertices, faces):
    """vertices float32 [V,3], faces integer [F,3] (numpy or tensors of one device) -> tri_data float32 [F,12]: the rows (v0, 0),
    (e1 = v1 - v0, 0), (e2 = v2 - v0, 0), each difference one float32 subtraction"""
    xp = torch if isinstance(vertices, torch.Tensor) else np
    idx = faces.long() if xp is torch else faces.astype(np.int64)
    v0, v1, v2 = vertices[idx[:, 0]], vertices[idx[:, 1]], vertices[idx[:, 2]]
    if xp is torch:
        out = torch.zeros(idx.shape[0], 12, dtype=torch.float32, device=vertices.device)
    else:
        out = np.zeros((idx.shape[0], 12), dtype=_f32)
    out[:, 0:3], out[:, 4:7], out[:, 8:11] = v0, v1 - v0, v2 - v0
    return out


def pack_vertices(vertices, faces):
    """vertices float32 [V,3], faces integer [F,3] (numpy or tensors of one device) -> tri_verts float32 [F,12]: the rows (v0, 0),
    (v1, 0), (v2, 0) of the exact vertices, the closest-point rule's table"""
    xp = torch if isinstance(vertices, torch.Tensor) else np
    idx = faces.long() if xp is torch else faces.astype(np.int64)
    if xp is torch:
        out = torch.zeros(idx.shape[0], 12, dtype=torch.float32, device=vertices.device)
    else:
        out = np.zeros((idx.shape[0], 12), dtype=_f32)
    out[:, 0:3], out[:, 4:7], out[:, 8:11] = vertices[idx[:, 0]], vertices[idx[:, 1]], vertices[idx[:, 2]]
    return out


def triangle_cells(tri_data, g):
    """numpy: the inclusive cell range of every triangle's grown bounding box -> (c0, c1) int64 [F,3]; k_bin_count's arithmetic"""
    t = np.asarray(tri_data, _f32)
    v0, a, b = t[:, 0:3], t[:, 0:3] + t[:, 4:7], t[:, 0:3] + t[:, 8:11]
    lo, hi = np.minimum(v0, np.minimum(a, b)), np.maximum(v0, np.maximum(a, b))
    top = (g["n"] - 1).astype(_f32)
    with np.errstate(all="ignore"):
        c0 = np.floor(((lo - g["grow"]) - g["lo"]) * g["inv_cell"])
        c1 = np.floor(((hi + g["grow"]) - g["lo"]) * g["inv_cell"])
    c0 = np.minimum(np.fmax(c0, _f32(0)), top).astype(np.int64)
    c1 = np.maximum(np.minimum(np.fmax(c1, _f32(0)), top).astype(np.int64), c0)
    return c0, c1


def bin_triangles_numpy(tri_data, g):
    """the kernels' binning in numpy -> (cell_start int32 [cells + 1], pair_tri int32 [P]): cell c's triangles are
    pair_tri[cell_start[c]:cell_start[c + 1]], ascending; cells in C order"""
    c0, c1 = triangle_cells(tri_data, g)
    span = c1 - c0 + 1
    counts = span.prod(1)
    P = int(counts.sum())
    if P >= 2 ** 31:
        raise ValueError(f"MeshWorld: {P} (cell, triangle) pairs do not fit int32 indices; use a coarser grid")
    tri = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    j = np.arange(P, dtype=np.int64) - np.repeat(np.cumsum(counts) - counts, counts)
    sy, sz = span[tri, 1], span[tri, 2]
    x, y, z = c0[tri, 0] + j // (sy * sz), c0[tri, 1] + (j // sz) % sy, c0[tri, 2] + j % sz
    cell = (x * g["n"][1] + y) * g["n"][2] + z
    order = np.argsort(cell, kind="stable")
    n_cells = int(np.prod(g["n"]))
    cell_start = np.searchsorted(cell[order], np.arange(n_cells + 1)).astype(np.int32)
    return cell_start, tri[order].astype(np.int32)


# ------------------------------------------------------------------------------------------------------------- the numpy path
def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def hit_terms(o, d, tri_data, dtype=_f32):
    """the hit rule's det, u, v, t for every (ray, triangle): o, d [R,3], tri_data [F,12] -> four [R,F] arrays of `dtype` (float32:
    the rule itself; float64: the same formulas, for error measurements)"""
    o, d, T = np.asarray(o, dtype), np.asarray(d, dtype), np.asarray(tri_data, dtype)
    oc, dc = [o[:, None, k] for k in range(3)], [d[:, None, k] for k in range(3)]
    v0, e1, e2 = [T[None, :, k] for k in range(0, 3)], [T[None, :, k] for k in range(4, 7)], [T[None, :, k] for k in range(8, 11)]
    with np.errstate(all="ignore"):
        p = _cross(dc, e2)
        det = _dot(e1, p)
        inv = dtype(1.0) / det
        s = [oc[k] - v0[k] for k in range(3)]
        u = _dot(s, p) * inv
        q = _cross(s, e1)
        v = _dot(dc, q) * inv
        t = _dot(e2, q) * inv
    return det, u, v, t


def _closest(ok, t):
    """the closest accepted candidate of every ray: ok bool [R,P], t float32 [R,P] -> (hit bool [R], best float32 [R]: the smallest
    accepted t, +inf on a miss; prim int64 [R]: the lowest index among the closest)"""
    tm = np.where(ok, t, _f32(np.inf))
    best = tm.min(1)
    hit = ok.any(1)
    return hit, np.where(hit, best, _f32(np.inf)), np.argmax(ok & (tm == best[:, None]), 1)


def cast_numpy(o, d, tri_data, t_min=0.0, t_max=np.inf):
    """brute force by the hit rule, float32: o, d [N,3] -> {"t" float32 (+inf on a miss), "prim" int32 (-1), "u", "v" float32 (0)}"""
    o, d, tri_data = np.ascontiguousarray(o, _f32).reshape(-1, 3), np.ascontiguousarray(d, _f32).reshape(-1, 3), np.asarray(tri_data, _f32)
    N, F = o.shape[0], tri_data.shape[0]
    t_min, t_max = _f32(t_min), _f32(t_max)
    out = {"t": np.full(N, np.inf, _f32), "prim": np.full(N, -1, np.int32), "u": np.zeros(N, _f32), "v": np.zeros(N, _f32)}
    valid = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)
    chunk = max(1, _CHUNK_PAIRS // max(1, F))
    for i0 in range(0, N, chunk):
        sl = slice(i0, min(N, i0 + chunk))
        det, u, v, t = hit_terms(o[sl], d[sl], tri_data)
        with np.errstate(all="ignore"):
            ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= _f32(1.0)) & (t > t_min) & (t < t_max) & valid[sl, None]
        hit, out["t"][sl], prim = _closest(ok, t)
        rows = np.arange(prim.shape[0])
        out["prim"][sl] = np.where(hit, prim, -1)
        out["u"][sl] = np.where(hit, u[rows, prim], _f32(0))
        out["v"][sl] = np.where(hit, v[rows, prim], _f32(0))
    return out


def closest_pair_terms(pc, v0, v1, v2, dtype=_f32, want_point=True):
    """the closest-point rule's candidates for operands that broadcast against each other: pc, v0, v1, v2 lists of three arrays of
    `dtype` (the point, the exact vertices) -> (d2 (+inf: no candidate), point: three arrays, or None without want_point).  The one
    copy of the rule's arithmetic: closest_terms evaluates it on all (point, triangle) pairs in float32, the clearance rule per
    (corner, triangle) pair in float64."""
    inf, zero, one = dtype(np.inf), dtype(0), dtype(1)
    with np.errstate(all="ignore"):
        e1, e2 = [v1[k] - v0[k] for k in range(3)], [v2[k] - v0[k] for k in range(3)]
        s = [pc[k] - v0[k] for k in range(3)]
        n = _cross(e1, e2)
        nn, sn = _dot(n, n), _dot(s, n)
        b, c = _dot(_cross(s, e2), n) / nn, _dot(_cross(e1, s), n) / nn
        inside = (nn > 0) & (b >= 0) & (c >= 0) & (b + c <= one)
        g = [np.maximum(np.maximum(np.minimum(v0[k], np.minimum(v1[k], v2[k])) - pc[k], pc[k] - np.maximum(v0[k], np.maximum(v1[k], v2[k]))), zero)
             for k in range(3)]
        box2, plane2 = _dot(g, g), (sn * sn) / nn
        d2 = np.where(inside, np.where(plane2 >= box2, plane2, box2), inf)
        point = None
        if want_point:
            w = sn / nn
            point = [np.where(inside, pc[k] - w * n[k], zero) for k in range(3)]
        s1 = [pc[k] - v1[k] for k in range(3)]
        e12 = [v2[k] - v1[k] for k in range(3)]
        for ap, a, ab, end in ((s, v0, e1, v1), (s, v0, e2, v2), (s1, v1, e12, v2)):
            den = _dot(ab, ab)
            t = np.where(den == 0, zero, _dot(ap, ab) / den)
            t = np.where(t >= 0, t, zero)
            t = np.where(t <= one, t, one)
            r = [ap[k] - t * ab[k] for k in range(3)]
            sd = _dot(r, r)
            take = sd < d2
            d2 = np.where(take, sd, d2)
            if want_point:
                point = [np.where(take, np.where(t == one, end[k], a[k] + t * ab[k]), point[k]) for k in range(3)]
    return d2, point


def closest_terms(p, tri, dtype=_f32):
    """the closest-point rule's d2 and closest point for every (point, triangle) before acceptance: p [R,3], tri [F,3,3] (the exact
    vertices) -> (d2 [R,F] (+inf: no candidate), point 3 x [R,F]) of `dtype` (float32: the rule itself; float64: the same formulas,
    for error measurements)"""
    p, T = np.asarray(p, dtype), np.asarray(tri, dtype)
    pc = [p[:, None, k] for k in range(3)]
    v0, v1, v2 = [[T[None, :, j, k] for k in range(3)] for j in range(3)]
    d2, point = closest_pair_terms(pc, v0, v1, v2, dtype)
    return d2.astype(dtype), [c.astype(dtype) for c in point]


def closest_numpy(points, vertices, faces, max_distance=np.inf, dtype=_f32):
    """brute force by the closest-point rule: points [N,3] -> {"distance" [N] (+inf on a miss), "prim" int32 [N] (-1), "point" [N,3]
    (NaN)}.  dtype float32 is the rule; float64 evaluates the same formulas in double on the same float32 inputs."""
    max_distance = dtype(max_distance)
    if max_distance != max_distance:
        raise ValueError("closest_numpy: max_distance is NaN")
    p = np.ascontiguousarray(points, _f32).reshape(-1, 3)
    tri = np.asarray(vertices, _f32).reshape(-1, 3)[np.asarray(faces).astype(np.int64).reshape(-1, 3)]
    N, F = p.shape[0], tri.shape[0]
    out = {"distance": np.full(N, np.inf, dtype), "prim": np.full(N, -1, np.int32), "point": np.full((N, 3), np.nan, dtype)}
    valid = np.isfinite(p).all(1)
    chunk = max(1, _CLOSEST_CHUNK_PAIRS // max(1, F))
    for i0 in range(0, N, chunk):
        sl = slice(i0, min(N, i0 + chunk))
        d2, point = closest_terms(p[sl], tri, dtype)
        some, best, prim = _closest((d2 < dtype(np.inf)) & valid[sl, None], d2)
        with np.errstate(all="ignore"):
            distance = np.sqrt(best)
            hit = some & (distance <= max_distance)
        rows = np.arange(prim.shape[0])
        out["distance"][sl] = np.where(hit, distance, dtype(np.inf))
        out["prim"][sl] = np.where(hit, prim, -1)
        for k in range(3):
            out["point"][sl, k] = np.where(hit, point[k][rows, prim], dtype(np.nan))
    return out


def _headlight(n, d, ambient):
    """the shading rule's headlight: n, d three float32 [N] arrays each -> float32 [N]"""
    with np.errstate(all="ignore"):
        length = np.sqrt(_dot(n, n)) * np.sqrt(_dot(d, d))
        cosine = np.where(length > 0, np.minimum(np.abs(_dot(n, d)) / length, _f32(1.0)), _f32(0)).astype(_f32)
        return _f32(ambient) + (_f32(1.0) - _f32(ambient)) * cosine


def _lit(col, shade):
    """colours float32 [N,3] under the headlight, clamped to [0, 1]"""
    return np.minimum(np.maximum(col * shade[:, None], _f32(0)), _f32(1.0))


def _quantise(image):
    """the uint8 copy of float32 pixels"""
    return (np.clip(image, 0, 1) * _f32(255.0)).astype(np.uint8)


def shade_numpy(d, prim, u, v, tri_data, faces, colors, bg, ambient):
    """the shading rule in numpy float32 (k_raycast_shade's bits) -> (image float32 [N,3], image_u8 uint8 [N,3])"""
    d, T = np.asarray(d, _f32).reshape(-1, 3), np.asarray(tri_data, _f32)
    prim = np.asarray(prim).reshape(-1)
    hit = prim >= 0
    f = np.where(hit, prim, 0)
    u, v = np.asarray(u, _f32).reshape(-1), np.asarray(v, _f32).reshape(-1)
    w = (_f32(1.0) - u) - v
    if colors is None:
        col = np.full((d.shape[0], 3), GREY, _f32)
    else:
        c = np.asarray(colors, _f32)[np.asarray(faces)[f].astype(np.int64)]           # [N, 3 corners, 3]
        col = (w[:, None] * c[:, 0] + u[:, None] * c[:, 1]) + v[:, None] * c[:, 2]
    e1, e2 = [T[f, k] for k in range(4, 7)], [T[f, k] for k in range(8, 11)]
    with np.errstate(all="ignore"):
        rgb = _lit(col, _headlight(_cross(e1, e2), [d[:, k] for k in range(3)], ambient))
    image = np.where(hit[:, None], rgb, np.asarray(bg, _f32)[None, :]).astype(_f32)
    return image, _quantise(image)


def _bg3(bg_color):
    bg = np.asarray(bg_color.detach().cpu().numpy() if isinstance(bg_color, torch.Tensor) else bg_color, _f32).reshape(-1)
    if bg.size == 1:
        bg = np.repeat(bg, 3)
    if bg.shape != (3,):
        raise ValueError("bg_color is a scalar or three values")
    return bg


# ------------------------------------------------------------------------------------------------------------- the overlay (numpy)
PRIM_CAPSULE, PRIM_BOX = 0.0, 1.0
_OVERLAY_CHUNK_PAIRS = 1 << 18                      # (ray, primitive) pairs per chunk of cast_overlay_numpy


def check_prims(prims):
    """the primitive table as float32 [P,8] numpy; ValueError for another shape, a kind other than 0 / 1, a non-finite field, r <= 0"""
    q = np.array(prims.detach().cpu().numpy() if isinstance(prims, torch.Tensor) else prims, dtype=_f32, order="C")       # (a copy)
    if q.size == 0:
        return q.reshape(0, 8)
    if q.ndim != 2 or q.shape[1] != 8:
        raise ValueError(f"overlay: the primitive table is [P,8] (kind, a.xyz, b.xyz, r), got {q.shape}")
    if q.shape[0] >= 2 ** 31:
        raise ValueError("overlay: P must be < 2^31")
    bad = ~np.isin(q[:, 0], (PRIM_CAPSULE, PRIM_BOX))
    if bad.any():
        raise ValueError(f"overlay: primitive {int(np.argmax(bad))} has kind {q[np.argmax(bad), 0]} (0: capsule, 1: box)")
    if not np.isfinite(q).all():
        raise ValueError(f"overlay: primitive {int(np.argmax(~np.isfinite(q).all(1)))} has a non-finite field")
    if not (q[:, 7] > 0).all():
        raise ValueError(f"overlay: primitive {int(np.argmax(~(q[:, 7] > 0)))} has r <= 0")
    return q


def overlay_prims(tubes=(), boxes=()):
    """tubes: (points [n,3], radius, rgb) each -- a polyline, n - 1 capsules (one point: a sphere);  boxes: (centres [m,3], half [3] or
    a scalar, rgb) each -- m axis-aligned boxes.  -> (prims float32 [P,8], colors float32 [P,3]), tubes first, in the given order"""
    rows, cols = [], []
    for points, radius, rgb in tubes:
        pts = np.asarray(points, _f32).reshape(-1, 3)
        if pts.shape[0] == 0:
            continue
        a, b = (pts[:-1], pts[1:]) if pts.shape[0] > 1 else (pts, pts)
        n = a.shape[0]
        rows.append(np.concatenate([np.full((n, 1), PRIM_CAPSULE, _f32), a, b, np.full((n, 1), radius, _f32)], 1))
        cols.append(np.tile(np.asarray(rgb, _f32).reshape(1, 3), (n, 1)))
    for centres, half, rgb in boxes:
        c = np.asarray(centres, _f32).reshape(-1, 3)
        n = c.shape[0]
        h = np.broadcast_to(np.asarray(half, _f32).reshape(-1), (3,)) if np.size(half) in (1, 3) else None
        if h is None:
            raise ValueError("overlay_prims: a box's half extents are a scalar or three values")
        rows.append(np.concatenate([np.full((n, 1), PRIM_BOX, _f32), c, np.tile(h[None], (n, 1)), np.ones((n, 1), _f32)], 1))
        cols.append(np.tile(np.asarray(rgb, _f32).reshape(1, 3), (n, 1)))
    if not rows:
        return np.zeros((0, 8), _f32), np.zeros((0, 3), _f32)
    return check_prims(np.concatenate(rows, 0)), np.ascontiguousarray(np.concatenate(cols, 0), _f32)


def overlay_terms(o, d, prims, recentre=True):
    """the overlay rule's t and normal for every (ray, primitive) before acceptance: o, d [R,3], prims [P,8] -> (t [R,P] (+inf: no
    candidate), normal 3 x [R,P]), float32.  recentre=False solves for o itself (t0 = 0): NOT the rule,
    the measurement DESIGN.md quotes as the reason for the re-centring."""
    o, d, q = np.asarray(o, _f32), np.asarray(d, _f32), np.asarray(prims, _f32)
    oc, dc = [o[:, None, k] for k in range(3)], [d[:, None, k] for k in range(3)]
    kind, a, b, r = q[None, :, 0], [q[None, :, 1 + k] for k in range(3)], [q[None, :, 4 + k] for k in range(3)], q[None, :, 7]
    capsule = kind == _f32(PRIM_CAPSULE)
    inf, zero = _f32(np.inf), _f32(0)
    with np.errstate(all="ignore"):
        dd = _dot(dc, dc)
        inv_dd = _f32(1.0) / dd

        def centred(c):
            t0 = _dot(dc, [c[k] - oc[k] for k in range(3)]) * inv_dd
            if not recentre:
                t0 = t0 * zero
            return t0, [(oc[k] + t0 * dc[k]) - c[k] for k in range(3)]

        # ---- capsule
        m = [(a[k] + b[k]) * _f32(0.5) for k in range(3)]
        t0, qm = centred(m)
        ba = [b[k] - a[k] for k in range(3)]
        oa = [qm[k] + (m[k] - a[k]) for k in range(3)]
        baba, rr = _dot(ba, ba), r * r
        u, w = _cross(ba, dc), _cross(ba, oa)
        A, B = _dot(u, u), _dot(u, w)
        C = _dot(w, w) - rr * baba
        h = B * B - A * C
        tp = (-B - np.sqrt(h)) / A
        y = _dot(ba, oa) + tp * _dot(ba, dc)
        body = (A > 0) & (h >= 0) & (y > 0) & (y < baba)
        t = np.where(body, t0 + tp, inf)
        n = [np.where(body, (oa[k] + tp * dc[k]) * baba - ba[k] * y, zero) for k in range(3)]
        for c in (a, b):
            t0, p = centred(c)
            Bs = _dot(dc, p)
            Cs = _dot(p, p) - rr
            hs = Bs * Bs - dd * Cs
            tp = (-Bs - np.sqrt(hs)) / dd
            tc = t0 + tp
            take = (hs >= 0) & (tc < t)
            t = np.where(take, tc, t)
            n = [np.where(take, p[k] + tp * dc[k], n[k]) for k in range(3)]
        # ---- box
        t0, pb = centred(a)
        t_near, t_far = np.full(t.shape, -np.inf, _f32), np.full(t.shape, np.inf, _f32)
        axis, miss = np.zeros(t.shape, np.int64), np.zeros(t.shape, bool)
        for k in range(3):
            still = dc[k] == 0
            miss |= still & (np.abs(pb[k]) > b[k])
            inv = _f32(1.0) / dc[k]
            t1, t2 = (-b[k] - pb[k]) * inv, (b[k] - pb[k]) * inv
            lo, hi = np.fmin(t1, t2), np.fmax(t1, t2)
            first = ~still & (lo > t_near)
            t_near = np.where(first, lo, t_near)
            axis = np.where(first, k, axis)
            t_far = np.where(still, t_far, np.fmin(t_far, hi))
        box_hit = ~miss & (t_near <= t_far)
        d_axis = np.where(axis == 0, dc[0], np.where(axis == 1, dc[1], dc[2]))
        sign = np.where(d_axis > 0, _f32(-1.0), _f32(1.0))
        nb = [np.where(box_hit & (axis == k), sign, zero) for k in range(3)]
        t = np.where(capsule, t, np.where(box_hit, t0 + t_near, inf))
        n = [np.where(capsule, n[k], nb[k]) for k in range(3)]
        return t.astype(_f32), [c.astype(_f32) for c in n]


def cast_overlay_numpy(o, d, prims, t_max=None, t_min=0.0):
    """the overlay rule, float32, chunked over (ray, primitive) pairs: o, d [N,3], prims [P,8], t_max [N] or None (+inf) ->
    {"t" float32 [N] (+inf on a miss), "prim" int32 [N] (-1), "normal" float32 [N,3] (0)}"""
    o, d = np.ascontiguousarray(o, _f32).reshape(-1, 3), np.ascontiguousarray(d, _f32).reshape(-1, 3)
    q = check_prims(prims)
    N, P = o.shape[0], q.shape[0]
    far = np.full(N, np.inf, _f32) if t_max is None else np.ascontiguousarray(t_max, _f32).reshape(-1)
    if far.shape[0] != N:
        raise ValueError("cast_overlay: t_max is one value per ray")
    t_min = _f32(t_min)
    out = {"t": np.full(N, np.inf, _f32), "prim": np.full(N, -1, np.int32), "normal": np.zeros((N, 3), _f32)}
    if P == 0 or N == 0:
        return out
    valid = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)
    chunk = max(1, _OVERLAY_CHUNK_PAIRS // P)
    for i0 in range(0, N, chunk):
        sl = slice(i0, min(N, i0 + chunk))
        t, n = overlay_terms(o[sl], d[sl], q)
        with np.errstate(all="ignore"):
            ok = (t > t_min) & (t < far[sl, None]) & valid[sl, None]
        hit, out["t"][sl], prim = _closest(ok, t)
        rows = np.arange(prim.shape[0])
        out["prim"][sl] = np.where(hit, prim, -1)
        for k in range(3):
            out["normal"][sl, k] = np.where(hit, n[k][rows, prim], _f32(0))
    return out


def shade_overlay_numpy(d, prim, normal, colors, ambient, image, image_u8):
    """k_overlay_shade in numpy float32: copies of image [N,3] / image_u8 [N,3] with the overlay's pixels written over"""
    d, n = np.asarray(d, _f32).reshape(-1, 3), np.asarray(normal, _f32).reshape(-1, 3)
    prim, col = np.asarray(prim).reshape(-1), np.asarray(colors, _f32).reshape(-1, 3)
    image, image_u8 = np.array(image, _f32).reshape(-1, 3), np.array(image_u8, np.uint8).reshape(-1, 3)
    hit = (prim >= 0) & (prim < col.shape[0])
    if not hit.any():
        return image, image_u8
    with np.errstate(all="ignore"):
        rgb = _lit(col[np.where(hit, prim, 0)], _headlight([n[:, k] for k in range(3)], [d[:, k] for k in range(3)], ambient))
    image[hit] = rgb[hit]
    image_u8[hit] = _quantise(rgb[hit])
    return image, image_u8


# ------------------------------------------------------------------------------------------------------------- the collision map
def signed_permutation(rot):
    """rot [3,3] -> (axis, sign) int [3] with w_i = sign[i] * x[axis[i]] = sum_j rot[i][j] x_j; ValueError unless rot is a signed
    permutation matrix (entries 0 or +-1, one non-zero per row and column)"""
    r = np.asarray(rot.detach().cpu().numpy() if isinstance(rot, torch.Tensor) else rot, dtype=np.float64)
    if r.shape != (3, 3) or not np.isin(r, (-1.0, 0.0, 1.0)).all() or (np.abs(r).sum(0) != 1).any() or (np.abs(r).sum(1) != 1).any():
        raise ValueError(f"voxelize: rot must be a signed permutation matrix (entries 0 or +-1, one per row and column), got {np.asarray(r).tolist()}")
    axis = np.abs(r).argmax(1)
    return axis.astype(np.int64), r[np.arange(3), axis].astype(np.int64)


def vertices_to_world(vertices, rot=PLANNER_ROT):
    """float32 vertices [V,3] in the NeRF's axes (numpy or tensor) -> the world frame, exactly: a copy or a negation per axis"""
    axis, sign = signed_permutation(rot)
    cols = [vertices[:, int(axis[a])] if sign[a] > 0 else -vertices[:, int(axis[a])] for a in range(3)]
    return torch.stack(cols, 1) if isinstance(vertices, torch.Tensor) else np.stack(cols, 1)


def check_voxel_box(box):
    """the boxes both paths accept: at least one cell per axis, fewer than 2^31 cells, and cells that float64 resolves (a box placed
    2^40 cells or more from the origin has none of the rule's arithmetic left)"""
    cells = int(np.prod([int(n) for n in box.shape], dtype=object)) if all(n >= 1 for n in box.shape) else 0
    if cells < 1 or cells >= 2 ** 31:
        raise ValueError(f"voxelize: the box needs at least one cell per axis and fewer than 2^31 cells (shape {box.shape})")
    g = box.granularity
    if not (g > 0 and np.isfinite(g) and np.isfinite(box.start).all()):
        raise ValueError(f"voxelize: the box needs a finite start and a positive finite granularity ({box})")
    reach = max(max(abs(s), abs(s + n / g)) for s, n in zip(box.start, box.shape))
    if not reach * g < 2.0 ** 40:
        raise ValueError(f"voxelize: the box lies 2^40 cells or more from the origin ({box})")


def face_candidates(vertices_world, faces, box):
    """the candidate cells of every face: per axis floor((min - start) g) - 1 .. floor((max - start) g) + 1 clipped to the box ->
    (lo int64 [F,3], n int64 [F,3]): the first cell and the number of cells (0: none); the face's cells in C order are its pairs"""
    tri = np.asarray(vertices_world, _f32)[np.asarray(faces).astype(np.int64)].astype(np.float64)          # [F, vertex, axis]
    start, g, top = np.asarray(box.start, np.float64), np.float64(box.granularity), np.asarray(box.shape, np.float64) - 1.0
    with np.errstate(all="ignore"):
        lo = np.floor((tri.min(1) - start) * g) - 1.0
        hi = np.floor((tri.max(1) - start) * g) + 1.0
    some = (hi >= 0.0) & (lo <= top)
    first = np.where(some, np.maximum(lo, 0.0), 0.0).astype(np.int64)
    last = np.where(some, np.minimum(hi, top), -1.0).astype(np.int64)
    return first, np.where(some, last - first + 1, 0)


def tri_box_overlap(tri, centre, h):
    """rule (a) for N (face, cell) pairs: tri float64 [N, vertex, axis] (world), centre float64 [N,3], h the half-width -> bool [N]"""
    p = tri - centre[:, None, :]
    out = np.zeros(tri.shape[0], dtype=bool)
    idx = np.nonzero(~((p.min(1) > h) | (p.max(1) < -h)).any(1))[0]               # the three box axes
    tri, p = tri[idx], p[idx]
    e = np.stack([tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 1], tri[:, 0] - tri[:, 2]], 1)         # [M, edge, axis]
    n = _cross([e[:, 0, a] for a in range(3)], [e[:, 1, a] for a in range(3)])
    d = _dot(n, [p[:, 0, a] for a in range(3)])
    sep = np.abs(d) > h * ((np.abs(n[0]) + np.abs(n[1])) + np.abs(n[2]))
    for j in range(3):
        ex, ey, ez = e[:, j, 0], e[:, j, 1], e[:, j, 2]
        for a1, a2, c1, c2 in ((-ez, ey, 1, 2), (ez, -ex, 0, 2), (-ey, ex, 0, 1)):             # u_0 x e, u_1 x e, u_2 x e
            q = a1[:, None] * p[:, :, c1] + a2[:, None] * p[:, :, c2]
            r = h * (np.abs(a1) + np.abs(a2))
            sep |= (q.min(1) > r) | (q.max(1) < -r)
    out[idx] = ~sep
    return out


def voxelize_numpy(vertices_world, faces, box, all_cells=False):
    """the voxelisation rule in numpy, chunked over (face, candidate cell) pairs: vertices_world float32 [V,3] (the world frame:
    vertices_to_world), faces integer [F,3], box a collision.GridBox -> bool [X,Y,Z].  all_cells: every cell of the box is every
    face's candidate (brute force, for small boxes: the candidates change no result)"""
    check_voxel_box(box)
    vw = np.ascontiguousarray(vertices_world, _f32).reshape(-1, 3)
    fc = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    shape = np.asarray(box.shape, np.int64)
    start, g = np.asarray(box.start, np.float64), np.float64(box.granularity)
    h = np.float64(0.5) / g
    occ = np.zeros(box.shape, dtype=bool)
    if fc.shape[0] == 0:
        return occ
    tri = vw[fc].astype(np.float64)
    with np.errstate(all="ignore"):
        cell = np.floor((tri.reshape(-1, 3) - start) * g)                          # rule (b): GridBox.indices' floor
    cell = cell[((cell >= 0) & (cell <= (shape - 1).astype(np.float64))).all(1)].astype(np.int64)
    occ[cell[:, 0], cell[:, 1], cell[:, 2]] = True
    if all_cells:
        lo, n = np.zeros((fc.shape[0], 3), np.int64), np.tile(shape, (fc.shape[0], 1))
    else:
        lo, n = face_candidates(vw, fc, box)
    counts = n.prod(1)
    ends = np.cumsum(counts)
    for p0 in range(0, int(ends[-1]), _VOXEL_CHUNK_PAIRS):
        pair = np.arange(p0, min(int(ends[-1]), p0 + _VOXEL_CHUNK_PAIRS), dtype=np.int64)
        f = np.searchsorted(ends, pair, side="right")                              # the first face with ends[f] > pair
        j = pair - (ends[f] - counts[f])
        nyz, nz = n[f, 1] * n[f, 2], n[f, 2]
        ijk = np.stack([lo[f, 0] + j // nyz, lo[f, 1] + (j % nyz) // nz, lo[f, 2] + j % nz], 1)
        centre = start + (ijk.astype(np.float64) + 0.5) / g
        hit = ijk[tri_box_overlap(tri[f], centre, h)]
        occ[hit[:, 0], hit[:, 1], hit[:, 2]] = True
    return occ


# ------------------------------------------------------------------------------------------------------------- the body (numpy)
_BODY_CHUNK_PAIRS = 1 << 18                         # (box, face) pairs per chunk of box_overlap_numpy


def check_boxes(boxes, who="box_overlap"):
    """the box table as float64 [N,15] numpy (a copy of nothing: a view where it can be); ValueError for another shape or N >= 2^31"""
    b = np.ascontiguousarray(boxes.detach().cpu().numpy() if isinstance(boxes, torch.Tensor) else boxes, np.float64)
    if b.size == 0 and (b.ndim < 2 or b.shape[-1] in (0, 15)):
        return b.reshape(0, 15)
    if b.ndim != 2 or b.shape[1] != 15:
        raise ValueError(f"{who}: the box table is [N,15] (centre, R row-major, half extents), got {b.shape}")
    if b.shape[0] >= 2 ** 31:
        raise ValueError(f"{who}: N must be < 2^31")
    return b


def box_parts(boxes):
    """boxes float64 [M,15] -> (c [M,3], R [M,3,3], h [M,3], valid bool [M]: every entry finite and no half extent negative)"""
    c, R, h = boxes[:, 0:3], boxes[:, 3:12].reshape(-1, 3, 3), boxes[:, 12:15]
    return c, R, h, np.isfinite(boxes).all(1) & (h >= 0).all(1)


def box_frame(c, R, x):
    """the body rule's x' = R^T (x - c): c [M,3], R [M,3,3], x [M,3] -> three [M] arrays, (R_0a d_0 + R_1a d_1) + R_2a d_2"""
    d = [x[:, k] - c[:, k] for k in range(3)]
    return [(R[:, 0, a] * d[0] + R[:, 1, a] * d[1]) + R[:, 2, a] * d[2] for a in range(3)]


def box_extent(R, h):
    """the half extent of the boxes' world bounds, E_a = (|R_a0| h_0 + |R_a1| h_1) + |R_a2| h_2 -> [M,3]"""
    A = np.abs(R)
    return (A[:, :, 0] * h[:, 0:1] + A[:, :, 1] * h[:, 1:2]) + A[:, :, 2] * h[:, 2:3]


def box_tri_overlap(boxes, tri):
    """the body rule's box-triangle test for M (box, face) pairs: boxes float64 [M,15], tri float64 [M, vertex, axis] (world) -> bool [M]"""
    out = np.zeros(boxes.shape[0], dtype=bool)
    with np.errstate(all="ignore"):
        c, R, h, valid = box_parts(boxes)
        p = np.stack([np.stack(box_frame(c, R, tri[:, k]), -1) for k in range(3)], 1)                  # [M, vertex, axis]
        idx = np.nonzero(valid & ~((p > h[:, None, :]).all(1) | (p < -h[:, None, :]).all(1)).any(1))[0]    # the three box axes
        p, h = p[idx], h[idx]
        e = np.stack([p[:, 1] - p[:, 0], p[:, 2] - p[:, 1], p[:, 0] - p[:, 2]], 1)                     # [M', edge, axis]
        n = _cross([e[:, 0, a] for a in range(3)], [e[:, 1, a] for a in range(3)])
        d = _dot(n, [p[:, 0, a] for a in range(3)])
        sep = np.abs(d) > (h[:, 0] * np.abs(n[0]) + h[:, 1] * np.abs(n[1])) + h[:, 2] * np.abs(n[2])
        for j in range(3):
            ex, ey, ez = e[:, j, 0], e[:, j, 1], e[:, j, 2]
            for a1, a2, c1, c2 in ((-ez, ey, 1, 2), (ez, -ex, 0, 2), (-ey, ex, 0, 1)):                 # u_0 x e, u_1 x e, u_2 x e
                q = a1[:, None] * p[:, :, c1] + a2[:, None] * p[:, :, c2]
                r = (h[:, c1] * np.abs(a1) + h[:, c2] * np.abs(a2))[:, None]
                sep |= (q > r).all(1) | (q < -r).all(1)
    out[idx] = ~sep
    return out


def box_overlap_numpy(boxes, vertices_world, faces):
    """the body rule's box-triangle test in numpy, brute force over all (box, face) pairs, chunked: boxes float64 [N,15],
    vertices_world float32 [V,3] (the world frame: vertices_to_world), faces integer [F,3] -> {"prim": int32 [N]}: the lowest
    index of an overlapping face, -1 without one"""
    b = check_boxes(boxes, "box_overlap_numpy")
    vw = np.ascontiguousarray(vertices_world, _f32).reshape(-1, 3)
    fc = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    N, F = b.shape[0], fc.shape[0]
    prim = np.full(N, -1, np.int32)
    if N == 0 or F == 0:
        return {"prim": prim}
    tri = vw[fc].astype(np.float64)
    chunk = max(1, _BODY_CHUNK_PAIRS // F)
    for i0 in range(0, N, chunk):
        part = b[i0:i0 + chunk]
        c, R, h, valid = box_parts(part)
        # the three box axes for every pair of the chunk, by broadcasting (box_frame's arithmetic); the few pairs they do not separate
        # go through the whole test
        keep = np.repeat(valid[:, None], F, 1)
        with np.errstate(all="ignore"):
            d = [[tri[None, :, k, j] - c[:, None, j] for j in range(3)] for k in range(3)]
            for a in range(3):
                p = [(R[:, None, 0, a] * d[k][0] + R[:, None, 1, a] * d[k][1]) + R[:, None, 2, a] * d[k][2] for k in range(3)]
                ha = h[:, None, a]
                keep &= ~(((p[0] > ha) & (p[1] > ha) & (p[2] > ha)) | ((p[0] < -ha) & (p[1] < -ha) & (p[2] < -ha)))
        bi, fi = np.nonzero(keep)
        hit = np.zeros(keep.shape, dtype=bool)
        hit[bi, fi] = box_tri_overlap(part[bi], tri[fi])
        prim[i0:i0 + part.shape[0]] = np.where(hit.any(1), hit.argmax(1), -1)
    return {"prim": prim}


# ------------------------------------------------------------------------------------------------------ the clearance (numpy)
CLEARANCE_SKIP = 2.0 ** -40                         # the margin of the clearance rule's lower-bound skip (the docstring's "Candidates")


def _clamp01(x):
    x = np.where(x >= 0, x, 0.0)
    return np.where(x <= 1, x, 1.0)


def _take_smaller(best, cand):
    return np.where(cand < best, cand, best)


def check_max_distance(max_distance, who):
    """the clearance rule's max_distance as a float: +inf is allowed, NaN or a value <= 0 is a ValueError"""
    d = float(max_distance)
    if not d > 0.0:
        raise ValueError(f"{who}: max_distance is a length > 0 or +inf (got {max_distance!r})")
    return d


def clamp_gap2(x, h):
    """the clearance rule's point-box candidate: x three [M] arrays (box frame), h three [M] half extents (arrays or scalars) ->
    (g_0^2 + g_1^2) + g_2^2, g_a = |x_a| - h_a where that is > 0, else 0"""
    g = []
    for a in range(3):
        d = np.abs(x[a]) - h[a]
        g.append(np.where(d > 0, d, 0.0))
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]


def point_tri_d2(pc, v0, v1, v2):
    """the closest-point rule's d2 (closest_pair_terms, float64) for M (point, triangle) PAIRS: four lists of three [M] arrays"""
    return closest_pair_terms(pc, v0, v1, v2, np.float64, want_point=False)[0]


def box_edge_segment_d2(h, a, sb, sc, q0, w):
    """the clearance rule's segment-segment candidate, in the box's frame: the box edge along axis a through (sb h_b, sc h_c) (b, c =
    a + 1, a + 2 mod 3; sb, sc = -1.0 or 1.0) against the segment q0 + t w, 0 <= t <= 1.  h, q0, w: three [M] arrays each -> d2 [M]"""
    b_, c_ = (a + 1) % 3, (a + 2) % 3
    p1 = [None] * 3
    p1[a], p1[b_], p1[c_] = -h[a], sb * h[b_], sc * h[c_]
    L = h[a] + h[a]
    r = [p1[k] - q0[k] for k in range(3)]
    A, e, f = L * L, _dot(w, w), _dot(w, r)
    c, b = L * r[a], L * w[a]
    den = A * e - b * b
    s0 = np.where(den > 0, _clamp01((b * f - c * e) / den), 0.0)
    t0 = (b * s0 + f) / e
    low = (e == 0) | ~(t0 >= 0)
    high = ~low & (t0 > 1)
    t = np.where(low, 0.0, np.where(high, 1.0, t0))
    s1 = np.where(A == 0, 0.0, _clamp01(np.where(low, -c, b - c) / A))
    s = np.where(low | high, s1, s0)
    d = [None] * 3
    d[a] = (p1[a] + L * s) - (q0[a] + w[a] * t)
    d[b_] = p1[b_] - (q0[b_] + w[b_] * t)
    d[c_] = p1[c_] - (q0[c_] + w[c_] * t)
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def box_edges_segment_d2(h, q0, w, best):
    """`best` lowered by the twelve box edges (axis a = 0, 1, 2; then (sb, sc) = (-,-), (+,-), (-,+), (+,+)) against one segment"""
    for a in range(3):
        for m in range(4):
            best = _take_smaller(best, box_edge_segment_d2(h, a, 1.0 if m & 1 else -1.0, 1.0 if m & 2 else -1.0, q0, w))
    return best


def frame_gap2(lo, hi, h):
    """the lower bound of the clearance rule's skip: the squared gap between the bounds lo_a..hi_a (box frame, three [M] arrays each)
    and the box, and the scale m = sum_a (max(|lo_a|, |hi_a|) + h_a) its margin is taken from -> (lb2 [M], m [M])"""
    g, m = [], 0.0
    for a in range(3):
        g.append(np.maximum(np.maximum(lo[a] - h[a], -h[a] - hi[a]), 0.0))
        m = m + (np.maximum(np.abs(lo[a]), np.abs(hi[a])) + h[a])
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2], m


def _box_tri_terms(boxes, tri):
    """-> (d2 float64 [M] by the clearance rule, +inf for an invalid row; overlap bool [M] by the body rule)"""
    inf = np.float64(np.inf)
    with np.errstate(all="ignore"):
        c, R, h, valid = box_parts(boxes)
        over = box_tri_overlap(boxes, tri)
        hh = [h[:, a] for a in range(3)]
        p = [box_frame(c, R, tri[:, k]) for k in range(3)]                                              # p[vertex][axis]
        best = np.full(boxes.shape[0], inf)
        for k in range(3):                                                                              # 1. the vertices against the box
            best = _take_smaller(best, clamp_gap2(p[k], hh))
        for m in range(8):                                                                              # 2. the corners against the triangle
            corner = [hh[a] if (m >> a) & 1 else -hh[a] for a in range(3)]
            best = _take_smaller(best, point_tri_d2(corner, p[0], p[1], p[2]))
        for j in range(3):                                                                              # 3. the edges against the edges
            q0, q1 = p[j], p[(j + 1) % 3]
            best = box_edges_segment_d2(hh, q0, [q1[a] - q0[a] for a in range(3)], best)
    return np.where(valid, np.where(over, 0.0, best), inf), over & valid


def box_tri_distance2(boxes, tri):
    """the clearance rule's squared distance for M (box, face) pairs: boxes float64 [M,15], tri float64 [M, vertex, axis] (world) ->
    float64 [M]: 0 where the body rule says overlap, else the smallest of the 47 candidates; +inf for an invalid row"""
    return _box_tri_terms(np.ascontiguousarray(boxes, np.float64), np.asarray(tri, np.float64))[0]


def _clearance_result(d2, over, index, max_distance):
    """per box from its pairs: d2, over [n, C], index int64 [n, C] or [C] the candidates' indices in ascending order along C ->
    the rule's per-box result (distance, index, hit)"""
    n = d2.shape[0]
    index = np.broadcast_to(index, d2.shape)
    rows = np.arange(n)
    if d2.shape[1] == 0:
        return np.full(n, np.inf), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    best = d2.min(1)
    first = np.argmax(d2 == best[:, None], 1)
    hit = np.where(over.any(1), index[rows, np.argmax(over, 1)], -1)
    with np.errstate(all="ignore"):
        distance = np.sqrt(best)
        ok = (best < np.inf) & (distance <= max_distance)
    prim = np.where(hit >= 0, hit, np.where(ok, index[rows, first], -1))
    return np.where(ok, distance, np.inf), prim.astype(np.int32), hit.astype(np.int32)


def box_clearance_numpy(boxes, vertices_world, faces, max_distance=np.inf):
    """the clearance rule against a mesh in numpy, brute force over all (box, face) pairs, chunked: boxes float64 [N,15],
    vertices_world float32 [V,3] (the world frame), faces integer [F,3] -> {"distance" float64 [N] (+inf: nothing within
    max_distance), "prim" int32 [N] (-1), "hit" int32 [N]: box_overlap_numpy's prim}.  The only pairs left out are those the rule's
    lower-bound skip proves beyond max_distance."""
    max_distance = check_max_distance(max_distance, "box_clearance_numpy")
    b = check_boxes(boxes, "box_clearance_numpy")
    vw = np.ascontiguousarray(vertices_world, _f32).reshape(-1, 3)
    fc = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    N, F = b.shape[0], fc.shape[0]
    out = {"distance": np.full(N, np.inf), "prim": np.full(N, -1, np.int32), "hit": np.full(N, -1, np.int32)}
    if N == 0 or F == 0:
        return out
    tri = vw[fc].astype(np.float64)
    limit2 = np.float64(max_distance) * np.float64(max_distance)
    chunk = max(1, _BODY_CHUNK_PAIRS // F)
    for i0 in range(0, N, chunk):
        part = b[i0:i0 + chunk]
        c, R, h, valid = box_parts(part)
        with np.errstate(all="ignore"):
            d = [[tri[None, :, k, j] - c[:, None, j] for j in range(3)] for k in range(3)]
            lo, hi = [], []
            for a in range(3):
                p = [(R[:, None, 0, a] * d[k][0] + R[:, None, 1, a] * d[k][1]) + R[:, None, 2, a] * d[k][2] for k in range(3)]
                lo.append(np.minimum(p[0], np.minimum(p[1], p[2])))
                hi.append(np.maximum(p[0], np.maximum(p[1], p[2])))
            lb2, m = frame_gap2(lo, hi, [h[:, None, a] for a in range(3)])
            keep = valid[:, None] & ~(lb2 > limit2 + CLEARANCE_SKIP * (limit2 + m * m))
        bi, fi = np.nonzero(keep)
        d2 = np.full(keep.shape, np.inf)
        over = np.zeros(keep.shape, dtype=bool)
        d2[bi, fi], over[bi, fi] = _box_tri_terms(part[bi], tri[fi])
        sl = slice(i0, i0 + part.shape[0])
        out["distance"][sl], out["prim"][sl], out["hit"][sl] = _clearance_result(d2, over, np.arange(F), max_distance)
    return out


def _voxel_box_struct(box, rot):
    axis, sign = signed_permutation(rot)
    b = _lib.VoxelBox()
    b.granularity = float(box.granularity)
    for a in range(3):
        b.start[a], b.shape[a], b.axis[a], b.sign[a] = float(box.start[a]), int(box.shape[a]), int(axis[a]), int(sign[a])
    return b


# ------------------------------------------------------------------------------------------------------------- the world
class MeshWorld:
    """A triangle mesh as the world a camera looks at.  vertices [V,3], faces integer [F,3], colors [V,3] (float in [0, 1], or uint8)
    or None (mid-grey): tensors (the mesh lives on their device) or numpy arrays (the CPU path).  frame="world": the vertices are in
    the planner's world frame and are turned into the NeRF's axes first (collision.to_nerf with PLANNER_ROT).
    Attributes: device, n_vertices, n_faces, grid (grid_params' dict), dims (nx, ny, nz), pairs, mean_pairs_per_cell, and the
    read-only tables tri_data, tri_verts, cell_start, pair_tri.  Shared freely between threads and streams: nothing is written after __init__."""

    def __init__(self, vertices, faces, colors=None, resolution=None, frame="nerf"):
        if frame not in ("nerf", "world"):
            raise ValueError(f"MeshWorld: frame is 'nerf' or 'world' (got {frame!r})")
        v = torch.as_tensor(np.asarray(vertices) if not isinstance(vertices, torch.Tensor) else vertices.detach())
        f = torch.as_tensor(np.asarray(faces) if not isinstance(faces, torch.Tensor) else faces.detach()).to(v.device)
        if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
            raise ValueError(f"MeshWorld: vertices [V,3] and faces [F,3] (got {tuple(v.shape)} and {tuple(f.shape)})")
        if v.shape[0] == 0 or f.shape[0] == 0:
            raise ValueError("MeshWorld: the mesh is empty")
        if f.shape[0] >= 2 ** 31 or v.shape[0] >= 2 ** 31:
            raise ValueError("MeshWorld: V and F must be < 2^31")
        if f.dtype.is_floating_point or f.dtype == torch.bool:
            raise ValueError("MeshWorld: faces are integer vertex indices")
        v = v.to(torch.float32)
        if frame == "world":
            v = to_nerf(v, PLANNER_ROT)
        v = v.contiguous()
        self.device = v.device
        f_lo, f_hi = int(f.min()), int(f.max())
        if f_lo < 0 or f_hi >= v.shape[0]:
            raise ValueError(f"MeshWorld: faces index outside the {v.shape[0]} vertices ({f_lo} .. {f_hi})")
        lo_hi = torch.stack([v.min(0).values, v.max(0).values]).cpu().numpy()
        if not np.isfinite(lo_hi).all():
            raise ValueError("MeshWorld: a vertex is not finite")
        self.vertices, self.faces = v, f.to(torch.int32).contiguous()
        self.n_vertices, self.n_faces = int(v.shape[0]), int(f.shape[0])
        if colors is not None:
            c = torch.as_tensor(np.asarray(colors) if not isinstance(colors, torch.Tensor) else colors.detach()).to(v.device)
            if tuple(c.shape) != (self.n_vertices, 3):
                raise ValueError(f"MeshWorld: colors [V,3] (got {tuple(c.shape)})")
            colors = (c.to(torch.float32) / 255.0 if c.dtype == torch.uint8 else c.to(torch.float32)).contiguous()
        self.colors = colors
        self.grid = grid_params(lo_hi[0], lo_hi[1], self.n_faces, resolution)
        self.dims = tuple(int(n) for n in self.grid["n"])
        self.tri_data = pack_triangles(self.vertices, self.faces)
        self.tri_verts = pack_vertices(self.vertices, self.faces)
        if self.device.type == "cuda":
            self._build_hip()
        else:
            cs, pt = bin_triangles_numpy(self.tri_data.numpy(), self.grid)
            self.cell_start, self.pair_tri = torch.from_numpy(cs), torch.from_numpy(pt)
        self.pairs = int(self.pair_tri.shape[0])
        self.mean_pairs_per_cell = self.pairs / float(np.prod(self.dims))

    def _build_hip(self):
        F = self.n_faces
        self._grid_c = _grid_struct(self.grid)
        n_cells = int(np.prod(self.dims))
        with torch.cuda.device(self.device):
            counts = torch.empty(F, dtype=torch.int32, device=self.device)
            _lib.call("raycast_bin_count", self.tri_data, F, ctypes.byref(self._grid_c), counts)
            ends = torch.cumsum(counts, 0, dtype=torch.int64)
            P = int(ends[-1])
            if P >= 2 ** 31:
                raise ValueError(f"MeshWorld: {P} (cell, triangle) pairs do not fit int32 indices; use a coarser grid")
            offsets = (ends - counts).contiguous()
            pair_cell = torch.empty(P, dtype=torch.int32, device=self.device)
            pair_tri = torch.empty(P, dtype=torch.int32, device=self.device)
            _lib.call("raycast_bin_emit", self.tri_data, F, ctypes.byref(self._grid_c), offsets, P, pair_cell, pair_tri)
            cells, order = torch.sort(pair_cell, stable=True)
            self.pair_tri = pair_tri[order].contiguous()
            self.cell_start = torch.searchsorted(cells, torch.arange(n_cells + 1, dtype=torch.int32, device=self.device)).to(torch.int32).contiguous()

    # ---- the collision map
    def occupancy(self, box, rot=PLANNER_ROT, pairs_per_launch=MAX_PAIRS_PER_LAUNCH):
        """the cells of `box` (a collision.GridBox, world frame) that the mesh's surface touches, by the module's voxelisation rule
        -> bool [X,Y,Z] on the world's device.  rot: the signed permutation that collision.to_nerf applied to the world's vertices
        (ValueError otherwise).  A HIP world runs on the current stream: a count kernel (one lane per face), torch.cumsum, the pair
        total read back (the only read), and the mark kernel (one lane per (face, candidate cell) pair) once per pairs_per_launch
        pairs -- a mesh with 2^31 pairs or more takes several launches; the map does not depend on that split."""
        check_voxel_box(box)
        if self.device.type != "cuda":
            vw = vertices_to_world(self.vertices.numpy(), rot)
            return torch.from_numpy(voxelize_numpy(vw, self.faces.numpy(), box))
        if not 1 <= int(pairs_per_launch) <= MAX_PAIRS_PER_LAUNCH:
            raise ValueError(f"MeshWorld.occupancy: pairs_per_launch is 1 .. {MAX_PAIRS_PER_LAUNCH}")
        b = _voxel_box_struct(box, rot)
        with torch.cuda.device(self.device):
            occ = torch.empty(box.shape, dtype=torch.uint8, device=self.device)
            counts = torch.empty(self.n_faces, dtype=torch.int32, device=self.device)
            _lib.call("voxelize_count", self.vertices, self.n_vertices, self.faces, self.n_faces, ctypes.byref(b), occ, counts)
            ends = torch.cumsum(counts, 0, dtype=torch.int64)
            pairs = int(ends[-1])
            for base in range(0, pairs, int(pairs_per_launch)):
                _lib.call("voxelize_mark", self.vertices, self.n_vertices, self.faces, self.n_faces, ctypes.byref(b), ends, base,
                          min(int(pairs_per_launch), pairs - base), occ)
        return occ.view(torch.bool)

    # ---- the body
    def box_overlap(self, boxes, rot=PLANNER_ROT):
        """boxes float64 [N,15] (the module's box table, world frame: collision.body_boxes) -> {"prim": int32 [N]}, the lowest index
        of a triangle each box overlaps by the module's body rule, -1 without one -- a tensor on the world's device (a numpy array
        for numpy boxes on a CPU world).  rot: the signed permutation that collision.to_nerf applied to the world's vertices
        (ValueError otherwise).  A HIP world runs csrc/body.hip on the current stream (one launch, no host read); a CPU world
        box_overlap_numpy."""
        tensors = isinstance(boxes, torch.Tensor)
        axis, sign = signed_permutation(rot)
        if self.device.type != "cuda":
            prim = box_overlap_numpy(check_boxes(boxes, "MeshWorld.box_overlap"), vertices_to_world(self.vertices.numpy(), rot), self.faces.numpy())["prim"]
            return {"prim": torch.from_numpy(prim) if tensors else prim}
        b = boxes.detach() if tensors else torch.from_numpy(check_boxes(boxes, "MeshWorld.box_overlap"))
        if b.dim() != 2 or b.shape[1] != 15:
            raise ValueError(f"MeshWorld.box_overlap: the box table is [N,15] (centre, R row-major, half extents), got {tuple(b.shape)}")
        b = b.to(self.device, torch.float64).contiguous()
        N = b.shape[0]
        if N >= 2 ** 31:
            raise ValueError("MeshWorld.box_overlap: N must be < 2^31")
        prim = torch.empty(N, dtype=torch.int32, device=self.device)
        if N:
            axis_c, sign_c = (ctypes.c_int32 * 3)(*[int(a) for a in axis]), (ctypes.c_int32 * 3)(*[int(s) for s in sign])
            with torch.cuda.device(self.device):
                _lib.call("box_mesh_overlap", b, N, ctypes.byref(self._grid_c), self.cell_start, self.pair_tri, self.pairs, self.tri_verts,
                          self.n_faces, ctypes.cast(axis_c, ctypes.c_void_p), ctypes.cast(sign_c, ctypes.c_void_p), prim)
        return {"prim": prim}

    def box_clearance(self, boxes, max_distance=float("inf"), rot=PLANNER_ROT):
        """boxes float64 [N,15] (box_overlap's table) -> {"distance" float64 [N], "prim" int32 [N], "hit" int32 [N]} by the module's
        clearance rule: the distance from each box to the nearest triangle (0 where they overlap, +inf where none lies within
        max_distance), the lowest index among the nearest (-1) and box_overlap's prim.  max_distance: a length > 0 or +inf
        (ValueError otherwise).  Tensors on the world's device (numpy arrays for numpy boxes on a CPU world).  A HIP world runs
        csrc/clearance.hip on the current stream (one launch, no host read); a CPU world box_clearance_numpy."""
        tensors = isinstance(boxes, torch.Tensor)
        max_distance = check_max_distance(max_distance, "MeshWorld.box_clearance")
        axis, sign = signed_permutation(rot)
        if self.device.type != "cuda":
            out = box_clearance_numpy(check_boxes(boxes, "MeshWorld.box_clearance"), vertices_to_world(self.vertices.numpy(), rot), self.faces.numpy(),
                                      max_distance)
            return {k: torch.from_numpy(v) for k, v in out.items()} if tensors else out
        b = boxes.detach() if tensors else torch.from_numpy(check_boxes(boxes, "MeshWorld.box_clearance"))
        if b.dim() != 2 or b.shape[1] != 15:
            raise ValueError(f"MeshWorld.box_clearance: the box table is [N,15] (centre, R row-major, half extents), got {tuple(b.shape)}")
        b = b.to(self.device, torch.float64).contiguous()
        N = b.shape[0]
        if N >= 2 ** 31:
            raise ValueError("MeshWorld.box_clearance: N must be < 2^31")
        out = {"distance": torch.empty(N, dtype=torch.float64, device=self.device), "prim": torch.empty(N, dtype=torch.int32, device=self.device),
               "hit": torch.empty(N, dtype=torch.int32, device=self.device)}
        if N:
            axis_c, sign_c = (ctypes.c_int32 * 3)(*[int(a) for a in axis]), (ctypes.c_int32 * 3)(*[int(s) for s in sign])
            with torch.cuda.device(self.device):
                _lib.call("box_mesh_clearance", b, N, ctypes.byref(self._grid_c), self.cell_start, self.pair_tri, self.pairs, self.tri_verts,
                          self.n_faces, ctypes.cast(axis_c, ctypes.c_void_p), ctypes.cast(sign_c, ctypes.c_void_p), max_distance,
                          out["distance"], out["prim"], out["hit"])
        return out

    # ---- the closest point of the surface
    def closest(self, points, max_distance=float("inf"), coherent=None, tested=False):
        """points [..., 3] -> {"distance" float32 [...] (+inf on a miss), "prim" int32 [...] (-1), "point" float32 [..., 3] (NaN)} by the
        module's closest-point rule, on the world's device (numpy arrays for numpy points on a CPU world).  max_distance: beyond it a
        point is a miss -- and the search stops there, which is what keeps points far from the surface cheap.  coherent: sort the
        queries by grid cell for the launch (None: from COHERENT_MIN_POINTS points on); a scheduling hint of the HIP path, the result
        does not depend on it.  tested=True (HIP only) adds "tested" int32 [...]: the (point, triangle) pairs evaluated."""
        max_distance = float(max_distance)
        if max_distance != max_distance:
            raise ValueError("MeshWorld.closest: max_distance is NaN")
        tensors = isinstance(points, torch.Tensor)
        p = (points.detach() if tensors else torch.from_numpy(np.array(points, dtype=_f32))).to(self.device, torch.float32)
        if p.dim() < 1 or p.shape[-1] != 3:
            raise ValueError(f"MeshWorld.closest: points [..., 3] (got {tuple(p.shape)})")
        shape = tuple(p.shape[:-1])
        p = p.reshape(-1, 3).contiguous()
        N = p.shape[0]
        if N >= 2 ** 31:
            raise ValueError("MeshWorld.closest: N must be < 2^31")
        if self.device.type != "cuda":
            if tested:
                raise ValueError("MeshWorld.closest: tested=True counts the HIP search's pairs; a CPU world tests all of them")
            out = closest_numpy(p.numpy(), self.vertices.numpy(), self.faces.numpy(), max_distance)
        else:
            out = {"distance": torch.empty(N, dtype=torch.float32, device=self.device), "prim": torch.empty(N, dtype=torch.int32, device=self.device),
                   "point": torch.empty(N, 3, dtype=torch.float32, device=self.device)}
            if tested:
                out["tested"] = torch.empty(N, dtype=torch.int32, device=self.device)
            if N:
                order = None
                if coherent if coherent is not None else N >= COHERENT_MIN_POINTS:
                    order = torch.argsort(self._cell_of(p), stable=True)
                    p = p[order].contiguous()
                raw = out if order is None else {k: torch.empty_like(a) for k, a in out.items()}
                with torch.cuda.device(self.device):
                    _lib.call("closest_point", p, N, ctypes.byref(self._grid_c), self.cell_start, self.pair_tri, self.pairs, self.tri_verts,
                              self.n_faces, max_distance, raw["distance"], raw["prim"], raw["point"], raw.get("tested"))
                if order is not None:
                    for k in out:
                        out[k][order] = raw[k]
        return {k: self._back(a, shape + (3,) if k == "point" else shape, tensors) for k, a in out.items()}

    def _cell_of(self, p):
        """the grid cell (C order) of each point clamped to the grid box, int64 [N]: the key `closest` sorts coherent queries by"""
        g = self.grid
        lo = torch.from_numpy(g["lo"]).to(p.device)
        n = torch.from_numpy(g["n"].astype(np.float32)).to(p.device)
        c = ((torch.nan_to_num(p, nan=0.0, posinf=0.0, neginf=0.0) - lo) * torch.from_numpy(g["inv_cell"]).to(p.device)).floor()
        c = torch.minimum(c.clamp_min(0.0), n - 1.0).to(torch.int64)
        return (c[:, 0] * int(g["n"][1]) + c[:, 1]) * int(g["n"][2]) + c[:, 2]

    # ---- casting
    def _flat(self, who, rays_d, rays_o=None):
        """what cast, shade and the overlay's two share on the way in: the directions [..., 3], with or without the origins ->
        (o or None, d: float32 [N,3], contiguous, on the world's device; the leading shape; whether the rays came as tensors)"""
        d = torch.as_tensor(rays_d).detach().to(self.device, torch.float32)
        o = None
        if rays_o is not None:
            o = torch.as_tensor(rays_o).detach().to(self.device, torch.float32)
            if o.shape != d.shape or o.dim() < 1 or o.shape[-1] != 3:
                raise ValueError(f"MeshWorld.{who}: rays_o and rays_d [..., 3] of one shape (got {tuple(o.shape)} and {tuple(d.shape)})")
            if o.numel() // 3 >= 2 ** 31:
                raise ValueError(f"MeshWorld.{who}: N must be < 2^31")
            o = o.reshape(-1, 3).contiguous()
        return o, d.reshape(-1, 3).contiguous(), tuple(d.shape[:-1]), isinstance(rays_d if rays_o is None else rays_o, torch.Tensor)

    @staticmethod
    def _width(who, frame_width, N):
        """the frame_width argument of the native casts (0: none)"""
        if frame_width is not None and (int(frame_width) < 1 or N % int(frame_width)):
            raise ValueError(f"MeshWorld.{who}: frame_width {frame_width} does not divide the {N} rays")
        return int(frame_width or 0)

    @staticmethod
    def _back(a, shape, tensors):
        """and on the way out: a flat per-ray result in `shape`, the rays' leading shape (+ (3,) for triples); a numpy result as a
        tensor for tensor rays"""
        a = a.reshape(shape)
        return torch.from_numpy(a) if tensors and isinstance(a, np.ndarray) else a

    def cast(self, rays_o, rays_d, t_min=0.0, t_max=float("inf"), frame_width=None):
        """rays [..., 3] -> {"t" float32 (+inf on a miss), "prim" int32 (-1), "u", "v" float32} of shape [...], on the world's device
        (numpy arrays for numpy rays on a CPU world).  frame_width: the rays are whole row-major frames of that width -- a
        scheduling hint of the HIP path (a wave takes an 8 x 8 pixel tile); the result does not depend on it."""
        t_min, t_max = float(t_min), float(t_max)
        if t_min != t_min or t_max != t_max:
            raise ValueError("MeshWorld.cast: t_min / t_max is NaN")
        o, d, shape, tensors = self._flat("cast", rays_d, rays_o)
        N = o.shape[0]
        width = self._width("cast", frame_width, N)
        if self.device.type != "cuda":
            out = cast_numpy(o.numpy(), d.numpy(), self.tri_data.numpy(), t_min, t_max)
        else:
            out = {"t": torch.empty(N, dtype=torch.float32, device=self.device), "prim": torch.empty(N, dtype=torch.int32, device=self.device),
                   "u": torch.empty(N, dtype=torch.float32, device=self.device), "v": torch.empty(N, dtype=torch.float32, device=self.device)}
            if N:
                with torch.cuda.device(self.device):
                    _lib.call("raycast", o, d, N, ctypes.byref(self._grid_c), self.cell_start, self.pair_tri, self.pairs, self.tri_data,
                              self.n_faces, t_min, t_max, width, out["t"], out["prim"], out["u"], out["v"])
        return {k: self._back(a, shape, tensors) for k, a in out.items()}

    def shade(self, rays_d, hit, bg_color=1.0, ambient=DEFAULT_AMBIENT):
        """a cast's result -> (image float32 [..., 3] in [0, 1], image_u8 uint8 [..., 3] = (uint8)(image * 255), Agent.get_img's
        quantisation) by the module's shading rule; bg_color (a scalar or three values; white, the reference's white_bg) on a miss"""
        if not 0.0 <= float(ambient) <= 1.0:
            raise ValueError("MeshWorld.shade: ambient must be in [0, 1]")
        bg = _bg3(bg_color)
        _, d, shape, tensors = self._flat("shade", rays_d)
        N = d.shape[0]
        prim, u, v = [torch.as_tensor(hit[k]).to(self.device).reshape(-1).contiguous() for k in ("prim", "u", "v")]
        if prim.shape[0] != N:
            raise ValueError("MeshWorld.shade: the hit record is not of these rays")
        if self.device.type != "cuda":
            image, u8 = shade_numpy(d.numpy(), prim.numpy(), u.numpy(), v.numpy(), self.tri_data.numpy(), self.faces.numpy(),
                                    None if self.colors is None else self.colors.numpy(), bg, ambient)
        else:
            image = torch.empty(N, 3, dtype=torch.float32, device=self.device)
            u8 = torch.empty(N, 3, dtype=torch.uint8, device=self.device)
            if N:
                bg_c = (ctypes.c_float * 3)(*[float(b) for b in bg])
                with torch.cuda.device(self.device):
                    _lib.call("raycast_shade", d, prim.to(torch.int32), u.to(torch.float32), v.to(torch.float32), N, self.tri_data,
                              self.faces, self.n_faces, self.colors, self.n_vertices, float(ambient), bg_c, image, u8)
        return self._back(image, shape + (3,), tensors), self._back(u8, shape + (3,), tensors)

    def _frame(self, pose, intrinsics, H, W, bg_color, ambient):
        """the mesh's part of a frame: nerf.utils.get_rays' rays of the pose, their cast and its shading -> (o, d, hit, image, image_u8)"""
        from .nerf.utils import get_rays
        pose = torch.as_tensor(pose).detach().to(self.device, torch.float32).reshape(1, 4, 4)
        rays = get_rays(pose, intrinsics, H, W)
        o, d = rays["rays_o"].reshape(-1, 3), rays["rays_d"].reshape(-1, 3)
        hit = self.cast(o, d, frame_width=W)
        return (o, d, hit) + self.shade(d, hit, bg_color, ambient)

    @staticmethod
    def _frame_dict(H, W, d, t, prim, image, u8):
        depth = t * torch.linalg.vector_norm(d, dim=-1)
        return {"image": image.reshape(H, W, 3), "image_u8": u8.reshape(H, W, 3), "depth": depth.reshape(H, W), "prim": prim.reshape(H, W)}

    def render(self, pose, intrinsics, H, W, bg_color=1.0, ambient=DEFAULT_AMBIENT):
        """pose [4,4] cam2world (this package's camera convention) -> {"image" float32 [H,W,3], "image_u8" uint8 [H,W,3], "depth"
        float32 [H,W] = t * |d| (+inf on a miss), "prim" int32 [H,W]} as tensors on the world's device.  The rays are
        nerf.utils.get_rays' of the pose: pixel-aligned with the NeRF's frame of the same pose."""
        _, d, hit, image, u8 = self._frame(pose, intrinsics, H, W, bg_color, ambient)
        return self._frame_dict(H, W, d, hit["t"], hit["prim"], image, u8)

    # ---- the overlay: analytic primitives drawn into the world (the replay's failure view)
    def cast_overlay(self, rays_o, rays_d, prims, t_max=None, t_min=0.0, frame_width=None):
        """rays [..., 3] against the primitive table prims [P,8] (the module's overlay rule) -> {"t" float32 (+inf on a miss), "prim"
        int32 (-1), "normal" float32 [..., 3] (unnormalised, 0 on a miss)} on the world's device (numpy arrays for numpy rays on a CPU
        world).  t_max: None (+inf) or the far limit per ray [...] -- a mesh cast's "t" of the same rays hides what lies behind the
        mesh.  frame_width: cast's scheduling hint; the result does not depend on it."""
        t_min = float(t_min)
        if t_min != t_min:
            raise ValueError("MeshWorld.cast_overlay: t_min is NaN")
        q = check_prims(prims)
        o, d, shape, tensors = self._flat("cast_overlay", rays_d, rays_o)
        N, P = o.shape[0], q.shape[0]
        width = self._width("cast_overlay", frame_width, N)
        far = None
        if t_max is not None:
            far = torch.as_tensor(t_max).detach().to(self.device, torch.float32).reshape(-1).contiguous()
            if far.shape[0] != N:
                raise ValueError("MeshWorld.cast_overlay: t_max is one value per ray")
        if self.device.type != "cuda":
            out = cast_overlay_numpy(o.numpy(), d.numpy(), q, None if far is None else far.numpy(), t_min)
        else:
            out = {"t": torch.empty(N, dtype=torch.float32, device=self.device), "prim": torch.empty(N, dtype=torch.int32, device=self.device),
                   "normal": torch.empty(N, 3, dtype=torch.float32, device=self.device)}
            if N:
                with torch.cuda.device(self.device):
                    q_dev = torch.from_numpy(q).to(self.device) if P else None
                    _lib.call("overlay_cast", o, d, N, q.ctypes.data if P else None, q_dev, P, t_min, far, width, out["t"], out["prim"],
                              out["normal"])
        return {k: self._back(a, shape + (3,) if k == "normal" else shape, tensors) for k, a in out.items()}

    def shade_overlay(self, rays_d, hit, colors, image, image_u8, ambient=DEFAULT_AMBIENT):
        """a cast_overlay result drawn over a frame: where the overlay hit, the pixel of `image` (float32 [..., 3]) and `image_u8`
        becomes colors[prim] (float [P,3]) times the shading rule's headlight on the hit's normal, with the same uint8 copy;
        every other pixel keeps its bits -> new (image, image_u8), the inputs are not written"""
        if not 0.0 <= float(ambient) <= 1.0:
            raise ValueError("MeshWorld.shade_overlay: ambient must be in [0, 1]")
        col = np.ascontiguousarray(colors.detach().cpu().numpy() if isinstance(colors, torch.Tensor) else colors, _f32).reshape(-1, 3)
        _, d, shape, _ = self._flat("shade_overlay", rays_d)
        tensors = isinstance(image, torch.Tensor)                       # (the frame decides what comes back, not the rays)
        N, P = d.shape[0], col.shape[0]
        prim = torch.as_tensor(hit["prim"]).to(self.device, torch.int32).reshape(-1).contiguous()
        normal = torch.as_tensor(hit["normal"]).to(self.device, torch.float32).reshape(-1, 3).contiguous()
        img = torch.as_tensor(image).to(self.device, torch.float32).reshape(-1, 3)
        u8 = torch.as_tensor(image_u8).to(self.device, torch.uint8).reshape(-1, 3)
        if prim.shape[0] != N or img.shape[0] != N or u8.shape[0] != N:
            raise ValueError("MeshWorld.shade_overlay: the hit record and the frame are not of these rays")
        if self.device.type != "cuda":
            img, u8 = shade_overlay_numpy(d.numpy(), prim.numpy(), normal.numpy(), col, ambient, img.numpy(), u8.numpy())
        else:
            img, u8 = img.clone().contiguous(), u8.clone().contiguous()
            if N and P:
                with torch.cuda.device(self.device):
                    _lib.call("overlay_shade", d, prim, normal, N, torch.from_numpy(col).to(self.device), P, float(ambient), img, u8)
        return self._back(img, shape + (3,), tensors), self._back(u8, shape + (3,), tensors)

    def render_scene(self, pose, intrinsics, H, W, tubes=(), boxes=(), bg_color=1.0, ambient=DEFAULT_AMBIENT):
        """render() with analytic primitives in the scene -- the replay's failure view.  tubes: (points [n,3], radius, rgb) each;
        boxes: (centres [m,3], half [3], rgb) each, in the mesh's axes (overlay_prims).  -> render's dict (image / image_u8 with the
        primitives drawn over the world where they are nearer than the mesh, depth the nearer of the two, prim the MESH's triangle) plus
        "overlay_prim" int32 [H,W]: the primitive's index (tubes first, in the given order), -1 where the mesh or the background
        shows.  Without primitives every entry equals render()'s bit for bit."""
        prims, colors = overlay_prims(tubes, boxes)
        o, d, hit, image, u8 = self._frame(pose, intrinsics, H, W, bg_color, ambient)
        over = self.cast_overlay(o, d, prims, t_max=hit["t"], frame_width=W)
        image, u8 = self.shade_overlay(d, over, colors, image, u8, ambient)
        return {**self._frame_dict(H, W, d, torch.minimum(hit["t"], over["t"]), hit["prim"], image, u8), "overlay_prim": over["prim"].reshape(H, W)}
