// stand-in for <hip/hip_runtime.h> and the rocPRIM headers on the host (tests/native/asmsum_emulate.cpp): what taxtree_emulate_hip.h
// has -- the block of 256 real threads, the stable-sort and scan stand-ins -- serves gs_asmsum.hip as it is
#pragma once
#include "taxtree_emulate_hip.h"
