/* The oracle's own conversion (planes_of, oracle/asm_oracle.c) behind one exported function, for host/pack_host_check.cpp: the oracle's
 * source is compiled into this unit as it is, so that the check compares with the very code the golden suite runs.  Test support only:
 * nothing in the product links this file. */
#include "../../oracle/asm_oracle.c"

/* out = { plane 0 low, plane 0 high, plane 1 low, plane 1 high } of a 128-byte buffer */
void pack_oracle_planes(const uint8_t* buf128, uint64_t* out) {
    v128 p0, p1;
    planes_of(buf128, &p0, &p1);
    out[0] = p0.lo, out[1] = p0.hi, out[2] = p1.lo, out[3] = p1.hi;
}
