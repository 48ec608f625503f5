// Library-internal view of a guard handle (guard.hip) for frame.hip; not part of the C-ABI.
#pragma once
#include "../../include/flope_amd.h"

// the FLOPE_DT_F16 engine the guard borrows; *slots: the guard's slot count (may be NULL)
extern "C" flope_handle flope_guard_fast_engine(flope_guard_handle g, int* slots);
// backbone_out_dim an engine was created with (engine.hip)
extern "C" int flope_engine_bod(flope_handle h);
// disarm a slot whose forward was enqueued but will not be repaired (waits for its count; FLOPE_OK also when the slot was idle)
extern "C" int flope_guard_cancel(flope_guard_handle g, int slot);
