/* rt_amd_rebuild.h — the part of the rt_amd.h ABI that rebuilds a device-built octree in place.  rt_amd.h includes it at its end, so a
 * program that includes rt_amd.h has these declarations; including this file alone works too.  The Python binding lists them in
 * rt_amd.SYMBOLS_REBUILD, and tests/test_rebuild_abi_host.py holds that table to this file as tests/test_host_and_abi.py holds
 * rt_amd.SYMBOLS to rt_amd.h.  RT_ABI_VERSION stays: these are additions. */
#ifndef RT_AMD_REBUILD_H
#define RT_AMD_REBUILD_H
#include "rt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The tree of an animated world, frame after frame, in ONE handle: rt_octree_rebuild_gpu rebuilds `octree` — a handle of
 * rt_build_octree_gpu — for the world's current device geometry (after rt_world_set_geometry), with the handle's own
 * spheres_per_leaf and precision.  After the call everything observable equals a fresh rt_build_octree_gpu(world, spl, &t, stream),
 * array for array and bit for bit: every rt_octree_debug_array by size and content, rt_octree_info / _nodes / _leaves / _flat_info /
 * _accel_info, and every frame, guide buffer and trace record rendered through the tree.  What it spares: the handle keeps the build's
 * workspace and the tree's two allocations, each with its capacity, and a rebuild lays its arrays out inside them — with capacities
 * that suffice it allocates and frees nothing — and it reads no array size back from the device: the count-dependent arrays run at the
 * length the handle holds (the last build's counts plus a quarter; the first rebuild of a handle allocates that slack once), the counts
 * stay on the device.  The host still waits where it decides something: for the median radius, which sets the grid's cell size, for
 * the registration totals, which set the lengths of the grid's two sorts, and at the end — at most 3 waits (binary16: 2) instead of 7.
 * A count that exceeds its length is found on the device (no kernel indexes by an unchecked count); the call then enlarges the memory
 * and runs once more from the start.
 *   - kept: the traversal mode (rt_octree_set_traversal).  The handle counts as a NEW tree for everything keyed on it: kept schedules,
 *     progressive tile orders and cached splits miss once, as they do after rt_free_octree + rt_build_octree_gpu;
 *   - ordering: the rebuild is ordered on `stream`; launches on other streams that still read the old tree are the caller's to order,
 *     as for rt_world_set_geometry.  The tree is ready to render when the call returns;
 *   - RT_EINVAL, the handle untouched: a NULL argument, a world whose num_spheres or precision is not the handle's, a handle of
 *     rt_build_octree (RT_BUILD_HOST).  A handle whose last build was RT_BUILD_HOST_DECLINED is accepted: the device is tried again;
 *   - the device build declines (see above): the tree is built on the host from the world's list, as rt_build_octree_gpu does, in
 *     this handle; rt_octree_build_path says RT_BUILD_HOST_DECLINED and the kept device memory is freed;
 *   - any other error after work has begun (RT_ENOMEM, a HIP error): the handle is left freeable — rt_free_octree succeeds — and
 *     renders nothing: no node, no grid, and the inspection calls refuse it.
 * rt_octree_rebuild_info (host only, diagnostics like the scheduling counters; any pointer may be NULL): rebuild calls that succeeded,
 * how many of them had to enlarge a piece of the kept memory or run twice, and the host-blocking waits of the last one. */
int rt_octree_rebuild_gpu(rt_octree* octree, const rt_world* world, void* stream);
int rt_octree_rebuild_info(const rt_octree* octree, uint64_t* rebuilds, uint64_t* regrown, uint64_t* host_syncs_last);

#ifdef __cplusplus
}
#endif
#endif /* RT_AMD_REBUILD_H */
