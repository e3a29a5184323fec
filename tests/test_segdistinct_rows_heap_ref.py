"""Collects the CPU cross-checks kept in segdistinct_rows_heap_ref.py (a helper module by its name): the model of
the resumed ordered segmented distinct over byte keys against oracle.DistinctRows, its slot invariants, and the
proof that the layout decides."""
from segdistinct_rows_heap_ref import (  # noqa: F401
    test_layout_decides_for_rows,
    test_model_is_the_oracle_and_its_state_ignores_the_cuts,
    test_slot_rule_by_hand,
)
