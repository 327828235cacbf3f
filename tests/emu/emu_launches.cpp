// emu_launches.cpp -- TEST INFRASTRUCTURE ONLY: the emulator build's launch record (lu_device.h, LU_EMU) for ctypes.
#include "../../lstm-unet_amd/csrc/lu_device.h"

// clear the record and start recording
extern "C" void lu_emu_launches_reset() {
    lu_launch_record::text.clear();
    lu_launch_record::on = true;
}

// copy the record (one kernel instance per line, as spelled at its launch site) into buf, NUL-terminated;
// returns the bytes the whole record needs (without the NUL), so a short buffer can be detected and retried
extern "C" size_t lu_emu_launches(char* buf, size_t cap) {
    const std::string& s = lu_launch_record::text;
    if (buf && cap) {
        const size_t n = s.size() < cap - 1 ? s.size() : cap - 1;
        memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return s.size();
}
