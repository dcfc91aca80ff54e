/* acn_device.h -- gfx950 device code of the trace / radiance path: the umbrella over its layers.  Every unit with a ray in it
 * includes this header (through acn_kernel_params.h, or by name); acn_records.h and acn_launch.h stop at base and scene, so the
 * units that trace nothing see none of the ray layers.
 *
 * What the reference does with recursion over heap objects and vtables (src/objects.c, src/compound.c,
 * src/scene.c:420-667) is done here with index-linked POD nodes, explicit per-lane stacks and state machines:
 *   - hit_machine   : obj_ray_hit over CSG trees (pair_inside / pair_outside / neg / scale wrappers) as a
 *                     coroutine-style state machine; all lanes of a wave that are "at a leaf" execute the same
 *                     plane / sphere / squaroid / SDF code together regardless of their depth in the tree.
 *   - side_machine  : obj_side as an iterative boolean-tree evaluation (short-circuited; children are pure).
 *   - compound walk : closest hit / any hit / transition hit over (nested) compounds with an explicit stack.
 *   - lum evaluator : scene_s_lum's branching recursion turned into a throughput-carrying work stack (pending
 *                     rays) plus a small stack of suspended path loops.
 * Floating-point expressions are written in the reference's order and compiled with -ffp-contract=off, so
 * geometry, seeds and control flow are bit-identical to the CPU oracle; only the radiance sums are
 * re-associated (throughput form), which moves colours by ~1e-16 relative.
 *
 * The layers, each a header of its own that includes what it needs (DESIGN.md section 4 has the table):
 *   acn_dev_base.h      DEV, the constants, V3 / M3, the address spaces, the vector functions, the LCGs and sampling
 *   acn_dev_scene.h     the LDS array, DevSceneT and its views, the counters, the phase timers, SceneRefT
 *   acn_dev_image.h     cl_sat, the camera ray and basis, the projection of a point             (base, scene)
 *   acn_dev_leaves.h    plane / sphere / squaroid / distance object, envelopes, roughness, pairs (base, scene)
 *   acn_dev_machines.h  the side machine and the hit machine, per lane and in lock step         (leaves)
 *   acn_dev_prune.h     the interval-prune programs                                             (leaves)
 *   acn_dev_traverse.h  compounds, element_hit, the root traversals and their fast forms        (machines, prune)
 *   acn_dev_shading.h   the cone of a light, the Oren-Nayar weights, the colour of an object    (leaves)
 */
#ifndef ACN_DEVICE_H
#define ACN_DEVICE_H

#include "acn_dev_base.h"
#include "acn_dev_scene.h"
#include "acn_dev_image.h"
#include "acn_dev_leaves.h"
#include "acn_dev_machines.h"
#include "acn_dev_prune.h"
#include "acn_dev_traverse.h"
#include "acn_dev_shading.h"

#endif /* ACN_DEVICE_H */
