"""The sub-batch plan of ``qoimi_encode_packed`` / ``qoimi_encode_images_packed`` as a pure function - the normative statement of what
qoi_stage_plan.h: pack_plan computes, so a caller (and the tests) can tell where the sub-batch boundaries of a call fall."""
from typing import List, Sequence, Tuple

SLOT_ALIGN = 256


def slot(bound: int) -> int:
    """Staging bytes of one image: its encode bound (``qoimi_encode_bound``) rounded up to 256."""
    return (int(bound) + SLOT_ALIGN - 1) // SLOT_ALIGN * SLOT_ALIGN


def plan(bounds: Sequence[int], staging_bytes: int) -> List[Tuple[int, int]]:
    """(first, count) of every sub-batch.  Images are taken in order; a sub-batch closes when the next slot would not fit in
    staging_bytes; a request smaller than a slot is raised to that slot, so no sub-batch is empty.  (The C entry points replace
    staging_bytes == 0 by their default before they plan; here 0 is just a very small request.)"""
    out, first, used = [], 0, 0
    for i, b in enumerate(bounds):
        s = slot(b)
        if i > first and used + s > staging_bytes:
            out.append((first, i - first))
            first, used = i, 0
        used += s
    if len(bounds):
        out.append((first, len(bounds) - first))
    return out
