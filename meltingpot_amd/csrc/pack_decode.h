// pack_decode.h — mp_create's host stage (pack_decode.hip): a pack decoded, checked, no HIP call.
#ifndef PACK_DECODE_H_
#define PACK_DECODE_H_

#include <vector>

#include "../../include/mp_pack.h"
#include "mp_common.h"

// Records the message mp_last_error returns (mp_engine.hip); returns `code`.
int fail(int code, const char* fmt, ...);

template <class T> struct MpkType;
template <> struct MpkType<uint8_t> { static constexpr uint32_t code = MPK_U8; };
template <> struct MpkType<char> { static constexpr uint32_t code = MPK_U8; };
template <> struct MpkType<int32_t> { static constexpr uint32_t code = MPK_I32; };
template <> struct MpkType<double> { static constexpr uint32_t code = MPK_F64; };
template <> struct MpkType<uint64_t> { static constexpr uint32_t code = MPK_U64; };
template <> struct MpkType<uint32_t> { static constexpr uint32_t code = MPK_U32; };

// Table `name` of element type T (NULL if absent or of another type); payloads
// are 16-byte aligned (mpk_validate), so int4 / uint4 reads of them are legal.
template <class T>
const T* table(const void* pack, const char* name, uint64_t* count = nullptr) {
  return static_cast<const T*>(mpk_require(pack, name, MpkType<T>::code, 0, count));
}

// What a pack decodes to: every table pointer is table_base + the table's offset in the
// pack; those the device stage owns (sprite_flags8, step_blob, fault, claim, atlas) NULL.
struct DecodedPack {
  DevTables t{};
  SubstrateTables sub{};   // (sub.mx.player_block: where the_matrix's MxPlayer block sits in a record)
  int nhits = 0;
  std::vector<uint8_t> extra;      // DevTables::sprite_flags8: sprite flags, state -> player, res_index
  std::vector<uint8_t> step_blob;  // DevTables::step_blob: the step kernels' LDS tables (step_common.h)
};

// A valid MPK1 pack of a supported substrate inside the engine's limits, holding
// cfg.num_players avatars; *hdr: its header table.
int check_header(const void* pack, uint64_t pack_len, const MpConfig& cfg, const int32_t** hdr);
// MpConfig.roles written into the host copy of a pack that passed check_header.
int apply_roles(std::vector<uint8_t>& pack, const MpConfig& cfg);
// Decodes and checks every table of a pack that passed check_header (MP_OK or MP_ERR_PACK);
// deterministic: calls with another table_base differ in the table pointers only.
int decode_pack(const std::vector<uint8_t>& pack, const MpConfig& cfg, const uint8_t* table_base,
                DecodedPack* out);

#endif  // PACK_DECODE_H_
