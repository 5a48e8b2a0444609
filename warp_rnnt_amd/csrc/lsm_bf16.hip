// lsm.h's forward log-softmax kernels for bf16 logits: fp32 from the load on (d/d logits: back once, at the store), same lanes,
// reduction tree and routing as fp32 -- bit-equal to the fp32 path on the upcast logits (d/d logits: that, rounded to E).
#include "lsm.h"

template struct rnnt::LsmOps<__bf16>;
