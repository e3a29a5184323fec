"""Collects the CPU cross-checks kept in segdistinct_rows_ref.py (a helper module by its name): the numpy
reference of the byte-key segmented-distinct GPU tests against oracle.DistinctRows."""
from segdistinct_rows_ref import (  # noqa: F401
    test_numpy_reference_equals_oracle_rows,
    test_numpy_uuid_hashcode_equals_oracle,
)
