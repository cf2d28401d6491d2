// What the facade drivers of tests/cpp share: a stand-in for libobs' obs_source_frame and whole-buffer file reads and writes.
#pragma once

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

struct fake_obs_source_frame            // the members of libobs' obs_source_frame the plugin's FrameIngest touches
{
    uint8_t* data[8] = {};
    uint32_t linesize[8] = {};
    uint32_t width = 0, height = 0;
    uint64_t timestamp = 0;
    int format = 0;
};

// fills buf from the head of the file: false unless it holds buf.size() bytes
inline bool read_file(const std::string& path, std::vector<uint8_t>& buf)
{
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    const bool ok = std::fread(buf.data(), 1, buf.size(), f) == buf.size();
    std::fclose(f);
    return ok;
}

inline bool write_file(const std::string& path, const std::vector<uint8_t>& buf)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    std::fclose(f);
    return ok;
}
