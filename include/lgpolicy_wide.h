/* lgpolicy_wide.h — C ABI of the wide observation row: an lg_mlp or an lg_rnn of lgpolicy.h whose INPUT is wider than the 512 columns every other
 * width is held to.  Same library, same error channel (lg_mlp_last_error), same handle types: what this header adds is one create function for the
 * MLP, and, through lgpolicy_wide_memory.h (included at the end), the one for the memory. */
#ifndef LGPOLICY_WIDE_H
#define LGPOLICY_WIDE_H
#include "lgpolicy.h"
#ifdef __cplusplus
extern "C" {
#endif

/* lg_mlp_create with an input row of up to LG_MLP_MAX_INPUT columns (an observation that carries a sensor: 66 + 512 rays); dims[1 .. num_layers]
 * stay 1..512.  The first layer of a handle with more than 512 inputs runs split-K: the row is staged in slabs of 512 columns and every output keeps
 * ONE k-ascending fp32 accumulator chain across the slabs, so the result does not depend on the slab size, and a network whose layer-0 weights are
 * zero from column 512 on gives the bits of the 512-input network.  For dims[0] <= 512 the handle is lg_mlp_create's: same kernels, same bits.
 * 2048 is four slabs, the tested bound (nothing in the kernels depends on the slab count).  Every entry point that runs the MLP on the caller's row
 * takes such a handle as it is: lg_mlp_forward, lg_policy_act, lg_distill_act, lg_collect_rollout, lg_collect_distillation, the lg_runner_collect*
 * family, lg_ppo_create and lg_distill_train_create.  The heads of the recurrent acts feed on their memory's hidden row (<= 512), so a head is never
 * wide; lg_estimator_step and the symmetric trainer refuse a wide lg_mlp by name.  NULL + "lg_mlp_create_wide: <which width, and its bound>" in
 * lg_mlp_last_error(NULL) otherwise, with nothing allocated. */
#define LG_MLP_MAX_INPUT 2048
lg_mlp* lg_mlp_create_wide(int32_t num_layers, const int32_t* dims, const float* const* weights, const float* const* biases,
                           int32_t activation, int device_id);

#ifdef __cplusplus
}
#endif
#include "lgpolicy_wide_memory.h"
#endif
