# cython: language_level=3
# distutils: language = c++
"""pyarrow.MemoryManager objects over gandiva::HipMemoryManager (gandiva/device_memory.h): the HBM of one GPU as an
Arrow memory domain.  `batch.copy_to(hip_memory_manager())` puts a RecordBatch there, `pyarrow.gandiva` projectors and
filters evaluate such a batch in place and allocate their outputs next to it, `array.copy_to(
pa.default_cpu_memory_manager())` brings a result back.  Built next to pyarrow's own gandiva.pyx by
build_pyarrow_gandiva.py."""
from libc.stdint cimport int64_t
from libcpp.memory cimport shared_ptr, static_pointer_cast
from pyarrow.lib cimport MemoryManager, check_status
from pyarrow.includes.common cimport CResult, CStatus, GetResultValue
from pyarrow.includes.libarrow cimport CMemoryManager


cdef extern from "gandiva/device_memory.h" namespace "gandiva" nogil:
    cdef cppclass CHipMemoryManager "gandiva::HipMemoryManager"(CMemoryManager):
        CStatus Trim()
        int64_t bytes_allocated(int64_t* in_use)

    cdef cppclass CHipDevice "gandiva::HipDevice":
        shared_ptr[CHipMemoryManager] hip_memory_manager()

    CResult[shared_ptr[CHipDevice]] CHipDevice_Make "gandiva::HipDevice::Make"(int device_id)


cdef shared_ptr[CHipMemoryManager] _manager(int device) except *:
    cdef shared_ptr[CHipDevice] dev = GetResultValue(CHipDevice_Make(device))
    return dev.get().hip_memory_manager()


def hip_memory_manager(int device=0):
    """The `pyarrow.MemoryManager` of library device `device` (gdv_set_device's numbering): one per device, it lives
    as long as the process."""
    return MemoryManager.wrap(static_pointer_cast[CMemoryManager, CHipMemoryManager](_manager(device)))


def reserved_bytes(int device=0):
    """(total, in_use): bytes the device's pool holds, and the part of them that live buffers occupy.  Buffers that
    were dropped stay in the pool (total - in_use) and serve the next allocation of their size."""
    cdef int64_t in_use = 0
    cdef int64_t total = _manager(device).get().bytes_allocated(&in_use)
    return total, in_use


def trim(int device=0):
    """Give the pool's retained (dropped, not yet reused) buffers back to the driver."""
    cdef shared_ptr[CHipMemoryManager] mm = _manager(device)
    with nogil:
        check_status(mm.get().Trim())
