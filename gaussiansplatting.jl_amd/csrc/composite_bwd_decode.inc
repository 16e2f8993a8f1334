// A staged entry as the backward walks read it.  Text, included by composite_bwd_visit.inc (the gradient visit of both walks) and
// by PASS 1 of composite_bwd_long_kernel, with C, the LDS planes l0..l3 (bwd_stage_entry), the slot j and the lane's fx in scope.
// Leaves a, b (planes 0 and 1), thr_bits (the blend threshold), o (opacity), dx and sx (the lane's column offset and the dx part
// of sigma), f[C] (the features) and entry_rowbits (the wave-uniform footprint mask: one bit per tile row in its low 16).
// (Text, not a function: returned as a struct or through reference arguments, every kernel of the tile walk carries the blend
// test's mask through a VGPR, +12 instructions — profiles/bwd_shared_visit/codegen_compare.txt.)  bench.py's hashes of the kernel
// sources, which mark profiles/pmc_traffic.json stale, cover composite.hip and not this file: after a change here, run
// tools/measure_pmc.sh again.
    const float4 a = l0[j], b = l1[j];
    const float4 t2 = l2[j];  // staged as (third colour, footprint mask, depth | :rgb blend threshold, slot)
    const float4 c2 = make_float4(t2.x, 0.0f, t2.z, t2.y);  // (x: third colour, w: footprint mask, z: depth) as the stream has them
    float4 t3 = t2;
    if (C > 3) t3 = l3[j];  // (normal xyz, blend threshold)
    const uint32_t thr_bits = __float_as_uint(C == 3 ? t2.z : t3.w);
    const float o = b.y;
    const float dx = a.x - fx;
    const SigmaX sx = sigma_x(a.z, a.w, dx);
    float f[C];
    unpack_features<C>(b, c2, t3, f);
    const uint32_t entry_rowbits = __builtin_amdgcn_readfirstlane(__float_as_uint(c2.w));
