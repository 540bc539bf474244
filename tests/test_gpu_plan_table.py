"""pal_plan_info / pal_plan_factors of the built library against the recorded table (tests/golden/plan_table.json): the wiring
from csrc/plan_geometry.h through Engine::get_plan to the C ABI.  The breadth is tests/test_host_plan_geometry.py's."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_table.json")
MAX_LENGTH = 1 << 20             # every recorded row (tests/test_gpu_long_frames.py builds plans of the longest frames anyway)


def test_plan_info_equals_the_recorded_table(monkeypatch):
    """One engine per switch set (the switches are read at creation), its plans dropped before the next set."""
    from pyaudiolocalization_amd import Engine
    with open(TABLE) as fh:
        table = json.load(fh)
    fields = table["fields"]
    assert sorted(table["sets"]) == sorted(["default", "PAL_RADIX3=0", "PAL_FOUR_REG=0", "PAL_PFA_BIG=0", "PAL_RADER=0", "PAL_PFA=0"])
    compared = 0
    for name, rows in table["sets"].items():
        if name != "default":
            monkeypatch.setenv(*name.split("="))
        eng = Engine(0)
        try:
            for length, want in rows.items():
                if int(length) > MAX_LENGTH:
                    continue
                info = eng.plan_info(int(length))
                assert [info[k] for k in fields] == want, (name, length, info)
                compared += 1
            eng.clear_plans()
        finally:
            eng.close()
            if name != "default":
                monkeypatch.delenv(name.split("=")[0])
    assert compared >= 120
